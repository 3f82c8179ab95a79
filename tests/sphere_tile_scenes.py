"""Scene texts of the sphere-interior tile tests (tests/test_sphere_interior_tiles.py on the host,
tests/test_gpu_sphere_tiles.py on the device): lecture5.sdl with a few lines changed so that a ball fills a small frame."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")

CSG_NODE = '    Node {\n      name      "csgNode"\n      geometry  "diff"\n      shader    "csg_shader"\n    }\n'
FLOOR_NODE = '    Node {\n      name      "floor"\n      geometry  "floor"\n      shader    "floor_shader"\n    }\n'
GLOBE_SHADER = 'Lambert {\n      name    "globe_shader"\n      texture "world"\n    }'
GLOBE_TEXTURE = 'BitmapTexture {\n      name  "world"\n      file  "world.bmp"\n    }'
LIGHT = "pos    -90 700 350"
LIT_BALL_LIGHT = "pos    -260 300 -100"     # above and behind the camera that looks at the moved ball: most of what it sees is lit
SELF_SHADOW_LIGHT = "pos    -200 300 900"  # behind the ball as the camera sees it: every visible point faces away from it


def texts():
    """dict of the scene texts; reads lecture5.sdl when called"""
    lecture5 = open(os.path.join(SCENES, "lecture5.sdl")).read()
    assert all(s in lecture5 for s in (CSG_NODE, FLOOR_NODE, GLOBE_SHADER, GLOBE_TEXTURE, LIGHT, "power  800000", "translate  100 15 156",
                                       "exponent  80"))
    base = lecture5.replace(CSG_NODE, "")  # (behind the eye the CsgDiff's box keeps the whole frame)
    # the camera 65 in front of the globe's centre; the three balls moved off to the left: under the globe they stay in the
    # shadow mask of most of its tiles
    globe = base.replace("pos    0 165 0", "pos    100 50 255").replace("pitch  -30", "pitch  0").replace("translate  100 15", "translate  -300 15")
    # the same view with the balls where they are
    globe_balls_under = base.replace("pos    0 165 0", "pos    100 50 255").replace("pitch  -30", "pitch  0")
    # the third ball (a node offset, Phong 80) alone at the side, the camera 20 in front of its centre: it fills the frame;
    # the light moved to the camera's side (where lecture5 has it, the whole visible cap faces away from it)
    ball = base.replace("translate  100 15 156", "translate  -200 40 100").replace("pos    0 165 0", "pos    -200 40 80").replace("pitch  -30", "pitch  0").replace(LIGHT, LIT_BALL_LIGHT)
    # no light and no floor: the planner has no ground node, the globe is the only node the primary mask keeps
    a, b = globe.index("  Lights {"), globe.index("  Geometries {")
    no_light = (globe[:a] + "  Lights {\n  }\n\n" + globe[b:]).replace(FLOOR_NODE, "")
    return dict(lecture5=lecture5, base=base, globe=globe, globe_balls_under=globe_balls_under, ball=ball,
                ball_self_shadowed=ball.replace(LIT_BALL_LIGHT, SELF_SHADOW_LIGHT), no_light=no_light)
