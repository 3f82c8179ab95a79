# Build of the MI355X render path (libc2rt.so) and of the CPU oracle
# (oracle/libc2rt_oracle.so, test infrastructure).  `make -j8`.
#
# Arithmetic flags are part of the contract: no contraction (the reference's
# x86-64 code has separate mul/add), IEEE fp32 divide/sqrt, no fast-math.
HIPCC      ?= hipcc
CC         ?= gcc
ARCH       ?= gfx950
FPFLAGS    := -ffp-contract=off -fno-fast-math
HIPFLAGS   := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC $(FPFLAGS) -fhip-fp32-correctly-rounded-divide-sqrt \
              -Wall -Wno-unused-function -Wno-bitwise-instead-of-logical $(EXTRA_HIPFLAGS)
# Kernel units only.  Machine LICM hoists loop-invariant scalar and vector values out of the node / CSG
# stepping loops of a kernel that is already at its register budget: more values live across the loops,
# more SGPRs spilled to VGPR lanes.  Measured with it off (profiles/r02_variants.md): lecture5 4K 1 tap
# 0.389 -> 0.375 ms, zaphod DOF 5.23 -> 5.04 ms, depth-4 VGPR spills 90 -> 60.
# -phi-node-folding-threshold=4 (round 4; LLVM's default is 2): SimplifyCFG turns slightly larger two-way branches into
# selects.  The only one of ~25 code-generation options screened that helps (profiles/r04_variants.md step 8): the
# headline instance drops from 122 to 118 VGPRs and from 151 to 135 SGPRs spilled to VGPR lanes; lecture5 4K x5
# 1.016 -> 0.997 ms, 4K x1 0.255 -> 0.249, 8K x4 3.20 -> 3.14, 1080p 0.078 -> 0.077; planes-only and depth-4
# instances unchanged.  (6 / 8 / 16: 133 spilled, a little slower than 4; 3: no change.)  Speculating a few more
# side-effect-free fp64 operations does not change a bit of any frame (the suite is bit-identical either way).
KERNELFLAGS := -mllvm -disable-machine-licm -mllvm -phi-node-folding-threshold=4
# Per unit (= CSG nesting depth of the frame-kernel instances in it), on top of KERNELFLAGS: GVN's partial-redundancy
# elimination off and SimplifyCFG's bonus-instruction threshold at 4 (profiles/r04_variants.md step 10, same-call
# A/B): planes-only / depth-0 instances -1.1 ... -2.5 % (zaphod DOF 3.947 -> 3.905 ms, zaphod x4 0.483 -> 0.472,
# lecture4 1080p 134.4 -> 138.0 Gray/s), csg_stress cut to depth 2 / 3 / 4: 1.715 -> 1.664, 3.735 -> 3.50, 8.29 ->
# 8.14 ms.  The depth-1 instances (the headline) were 0.6 % slower with them at the time and went without; measured
# again after steps 12 - 17 had changed what those instances keep in registers they gain 1.9 % (0.925 -> 0.908 ms,
# 1080p +2.5 %; the threshold alone: 1.6 %) and the other depths still want theirs (step 18).  Kept per unit: the
# answer has changed once already.  Depth 4 also takes the scheduler's max-memory-clause strategy: those instances are
# latency-bound (VALU busy 0.64, 43 % of the wave-cycles waiting for memory) and gain 2.3 % from it (csg_stress 7.80 ->
# 7.62 ms; the other strategies 1.2 %); depth 3 LOSES 2.2 % with it, depth 2 and the issue-bound depths 0 / 1 do not
# care for it (step 20); depth 1 takes iterative-ilp, worth 0.6 % on the headline frame; depth 2 iterative-ilp as well (-3 % on csg_stress cut
# to depth 2); depth 0 and depth 3 keep the default (depth 0: max-ilp gains 1.8 % on lecture4 1080p but puts 32 B of
# scratch into the depth-of-field planes instance; depth 3: every other strategy is slower).
KERNELFLAGS_u0 := -mllvm -enable-pre=false -mllvm -bonus-inst-threshold=4
KERNELFLAGS_u1 := -mllvm -enable-pre=false -mllvm -bonus-inst-threshold=4 -mllvm -amdgpu-sched-strategy=iterative-ilp
KERNELFLAGS_u2 := -mllvm -enable-pre=false -mllvm -bonus-inst-threshold=4 -mllvm -amdgpu-sched-strategy=iterative-ilp
KERNELFLAGS_u3 := -mllvm -enable-pre=false -mllvm -bonus-inst-threshold=4
KERNELFLAGS_u4 := -mllvm -enable-pre=false -mllvm -bonus-inst-threshold=4 -mllvm -amdgpu-sched-strategy=max-memory-clause
KERNELFLAGS_u5 :=
# the query kernels, one object per file, every CSG depth in it (exact:: only: a fraction of a frame unit's code) —
# c2rt_rays (ray / visibility queries, c2rt_trace_rays), c2rt_hit_planes (the hit planes of a camera frame,
# c2rt_render_hits), c2rt_layers (every surface along a ray or pixel, c2rt_trace_rays_layers / c2rt_render_hit_layers),
# c2rt_shade_planes (the terms of a sample's colour, c2rt_render_shading / c2rt_trace_rays_shading),
# c2rt_occlusion (hemisphere visibility of every hit, c2rt_render_occlusion / c2rt_trace_rays_occlusion),
# c2rt_gather (one-bounce indirect light of every hit, c2rt_render_gather / c2rt_trace_rays_gather),
# c2rt_paths (multi-bounce indirect light of every hit, c2rt_render_paths / c2rt_trace_rays_paths),
# c2rt_paths_counted (the same with a path count per sample, c2rt_render_paths_counted / c2rt_trace_rays_paths_counted),
# c2rt_adaptive (adaptive anti-aliasing, c2rt_render_frame_adaptive: detection and refinement),
# c2rt_sample_taps (frames and adaptive refinement over a caller's tap table, c2rt_render_frame_taps); the
# flags of the frame units were tuned on the frame kernels and have not been measured here
KERNELFLAGS_QUERY :=
# c2rt_denoise (the a-trous filter, c2rt_denoise*): an fp32 stencil that traces nothing and includes none of the trace
# headers; the arithmetic flags only, none of the code-generation flags above
# c2rt_temporal (the temporal accumulation, c2rt_temporal_accumulate*): the same — a gather that traces nothing
# c2rt_denoise_variance (the variance-guided filter, c2rt_denoise_variance*): the same
# c2rt_path_counts (the count rule over the temporal history, c2rt_path_counts*): the same
CXXFLAGS   := -O2 -std=c++17 -fPIC $(FPFLAGS) -Wall -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include
CSRC       := chess2rt_amd/csrc
# development knob: `make VARIANT=name EXTRA_HIPFLAGS=... EXTRA_KERNEL_FLAGS=...` builds chess2rt_amd/libc2rt_name.so
# (EXTRA_KERNEL_FLAGS reach only the hipcc kernel units, e.g. -mllvm options)
VARIANT    ?=
BUILD      := build$(if $(VARIANT),_$(VARIANT))
LIBNAME    := chess2rt_amd/libc2rt$(if $(VARIANT),_$(VARIANT)).so

UNITS      := 0 1 2 3 4 5
QUERIES    := c2rt_rays c2rt_hit_planes c2rt_layers c2rt_shade_planes c2rt_occlusion c2rt_gather c2rt_paths c2rt_paths_counted c2rt_adaptive c2rt_sample_taps
KOBJS      := $(foreach u,$(UNITS),$(BUILD)/c2rt_kernels_u$(u).o) $(foreach q,$(QUERIES),$(BUILD)/$(q).o) $(BUILD)/c2rt_denoise.o $(BUILD)/c2rt_temporal.o $(BUILD)/c2rt_denoise_variance.o $(BUILD)/c2rt_path_counts.o
HOBJS      := $(BUILD)/c2rt_api.o $(BUILD)/scene_plan.o $(BUILD)/dsc.o $(BUILD)/scene.o $(BUILD)/host_api.o

# diagnostics build of the same library: c2rt_api.cpp with the environment hooks compiled in (-DC2RT_DIAG=1), linked
# over the SAME kernel objects; tests and scripts that need a hook load it with C2RT_LIB_VARIANT=diag
DIAGNAME   := chess2rt_amd/libc2rt_diag.so
# the same with the depth-1 frame unit's lane statistics compiled in (its rules are below, behind the diagnostics library's)
STATSNAME  := chess2rt_amd/libc2rt_lanestats.so

all: $(LIBNAME) $(if $(VARIANT),,$(DIAGNAME) $(STATSNAME)) oracle/libc2rt_oracle.so oracle/libc2rt_oracle_count.so tests/fp64_lean_check tests/certain_f32_check tests/libcsg_void_check.so tests/libsphere_cull_check.so tests/libscene_plan_check.so tests/libscene_update_check.so tests/libground_fast_check.so tests/libground_dark_check.so tests/libground_certain_check.so tests/libground_texel_check.so tests/libsphere_interior_check.so tests/libcsg_certain_check.so tests/libcsg_tile_check.so tests/tap_average_check

$(BUILD):
	mkdir -p $(BUILD)

# (the Makefile is a prerequisite: the arithmetic and code-generation flags are part of what a kernel object is)
TRACE_DEPS := $(CSRC)/c2rt_trace_common.inc $(CSRC)/c2rt_trace_shared.inc $(CSRC)/c2rt_tile_mask.inc $(CSRC)/c2rt_trace.inc $(CSRC)/c2rt_device.h $(CSRC)/csg_void.h $(CSRC)/csg_certain.h $(CSRC)/x87.h $(CSRC)/fp64_lean.h $(CSRC)/f32_certain.h $(CSRC)/ground_certain.h include/c2rt.h Makefile
$(BUILD)/c2rt_kernels_u%.o: $(CSRC)/c2rt_kernels.hip $(TRACE_DEPS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) $(KERNELFLAGS) $(KERNELFLAGS_u$*) $(EXTRA_KERNEL_FLAGS) -DC2RT_UNIT=$* -c $< -o $@

$(foreach q,$(QUERIES),$(BUILD)/$(q).o): $(BUILD)/%.o: $(CSRC)/%.hip $(CSRC)/c2rt_query.inc $(CSRC)/c2rt_query.h $(TRACE_DEPS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) $(KERNELFLAGS) $(KERNELFLAGS_QUERY) $(EXTRA_KERNEL_FLAGS) -c $< -o $@
$(BUILD)/c2rt_paths_counted.o: $(CSRC)/c2rt_paths_counted.h $(CSRC)/c2rt_temporal.h

$(BUILD)/c2rt_denoise.o: $(CSRC)/c2rt_denoise.hip $(CSRC)/c2rt_denoise.h include/c2rt.h Makefile | $(BUILD)
	$(HIPCC) $(HIPFLAGS) $(EXTRA_KERNEL_FLAGS) -c $< -o $@

$(BUILD)/c2rt_temporal.o: $(CSRC)/c2rt_temporal.hip $(CSRC)/c2rt_temporal.h include/c2rt.h Makefile | $(BUILD)
	$(HIPCC) $(HIPFLAGS) $(EXTRA_KERNEL_FLAGS) -c $< -o $@

$(BUILD)/c2rt_path_counts.o: $(CSRC)/c2rt_path_counts.hip $(CSRC)/c2rt_paths_counted.h $(CSRC)/c2rt_temporal.h $(CSRC)/c2rt_query.h $(CSRC)/c2rt_device.h include/c2rt.h Makefile | $(BUILD)
	$(HIPCC) $(HIPFLAGS) $(EXTRA_KERNEL_FLAGS) -c $< -o $@

$(BUILD)/c2rt_denoise_variance.o: $(CSRC)/c2rt_denoise_variance.hip $(CSRC)/c2rt_denoise_variance.h $(CSRC)/c2rt_denoise.h include/c2rt.h Makefile | $(BUILD)
	$(HIPCC) $(HIPFLAGS) $(EXTRA_KERNEL_FLAGS) -c $< -o $@

$(BUILD)/c2rt_api.o: $(CSRC)/c2rt_api.cpp $(CSRC)/c2rt_denoise.h $(CSRC)/c2rt_denoise_variance.h $(CSRC)/c2rt_temporal.h $(CSRC)/c2rt_paths_counted.h $(CSRC)/c2rt_query.h $(CSRC)/scene_plan.h $(CSRC)/c2rt_device.h $(CSRC)/csg_void.h $(CSRC)/ground_certain.h include/c2rt.h | $(BUILD)
	g++ $(CXXFLAGS) $(EXTRA_HIPFLAGS) -c $< -o $@

# the HIP-free planner (scene validation and packing, per-frame culling decisions)
$(BUILD)/scene_plan.o: $(CSRC)/scene_plan.cpp $(CSRC)/scene_plan.h $(CSRC)/c2rt_device.h $(CSRC)/csg_void.h $(CSRC)/ground_certain.h include/c2rt.h | $(BUILD)
	g++ $(CXXFLAGS) -c $< -o $@

$(BUILD)/%.o: $(CSRC)/host/%.cpp $(CSRC)/host/scene.hpp $(CSRC)/host/dsc.hpp include/c2rt.h include/c2rt_host.h | $(BUILD)
	g++ $(CXXFLAGS) -c $< -o $@

$(LIBNAME): $(KOBJS) $(HOBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^ -lpthread

$(BUILD)/c2rt_api_diag.o: $(CSRC)/c2rt_api.cpp $(CSRC)/c2rt_denoise.h $(CSRC)/c2rt_denoise_variance.h $(CSRC)/c2rt_temporal.h $(CSRC)/c2rt_paths_counted.h $(CSRC)/c2rt_query.h $(CSRC)/scene_plan.h $(CSRC)/c2rt_device.h $(CSRC)/csg_void.h $(CSRC)/ground_certain.h include/c2rt.h | $(BUILD)
	g++ $(CXXFLAGS) $(EXTRA_HIPFLAGS) -DC2RT_DIAG=1 -c $< -o $@

$(DIAGNAME): $(KOBJS) $(BUILD)/c2rt_api_diag.o $(filter-out $(BUILD)/c2rt_api.o,$(HOBJS))
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^ -lpthread

# lane-statistics build of the diagnostics library: the depth-1 frame unit and c2rt_api.cpp compiled with -DC2RT_TILE_STATS=1
# (the region and lane counters of c2rt_trace_shared.inc, c2rt_debug_set_tile_stats), linked over the SAME objects for
# everything else — one more compile of one unit.  tests/test_gpu_csg_certain.py reads the certain / unsure lane counts
# of csg_certain.h from it (C2RT_LIB_VARIANT=lanestats); frames of other CSG depths run the plain units and count nothing.
$(BUILD)/c2rt_kernels_u1_stats.o: $(CSRC)/c2rt_kernels.hip $(TRACE_DEPS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) $(KERNELFLAGS) $(KERNELFLAGS_u1) $(EXTRA_KERNEL_FLAGS) -DC2RT_TILE_STATS=1 -DC2RT_UNIT=1 -c $< -o $@

$(BUILD)/c2rt_api_stats.o: $(CSRC)/c2rt_api.cpp $(CSRC)/c2rt_denoise.h $(CSRC)/c2rt_denoise_variance.h $(CSRC)/c2rt_temporal.h $(CSRC)/c2rt_paths_counted.h $(CSRC)/c2rt_query.h $(CSRC)/scene_plan.h $(CSRC)/c2rt_device.h $(CSRC)/csg_void.h $(CSRC)/ground_certain.h include/c2rt.h | $(BUILD)
	g++ $(CXXFLAGS) $(EXTRA_HIPFLAGS) -DC2RT_DIAG=1 -DC2RT_TILE_STATS=1 -c $< -o $@

$(STATSNAME): $(filter-out $(BUILD)/c2rt_kernels_u1.o,$(KOBJS)) $(BUILD)/c2rt_kernels_u1_stats.o $(BUILD)/c2rt_api_stats.o $(filter-out $(BUILD)/c2rt_api.o,$(HOBJS))
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^ -lpthread

# device check of fp64_lean.h against the compiler's own divide / sqrt expansions (tests/test_gpu_parity.py runs it)
tests/fp64_lean_check: tests/fp64_lean_check.hip $(CSRC)/fp64_lean.h
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++17 $(FPFLAGS) -fhip-fp32-correctly-rounded-divide-sqrt $< -o $@

# device check of f32_certain.h and its two wrappers against the device's own atan2 / asin / pow and the x87 emulation
# (tests/test_gpu_f32_certain.py runs it)
tests/certain_f32_check: tests/certain_f32_check.hip $(TRACE_DEPS)
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 $(FPFLAGS) -fhip-fp32-correctly-rounded-divide-sqrt $< -o $@

# host build of the CsgDiff void-tile test of the mask pre-pass (tests/test_csg_void_tiles.py, scripts/csg_void_tiles.py)
tests/libcsg_void_check.so: tests/csg_void_check.cpp $(CSRC)/csg_void.h
	g++ -O2 -std=c++17 -fPIC -shared $(FPFLAGS) -Wall -o $@ $<

# host build of csg_certain.h, the per-lane decision of a leaf CsgOp's winning hit (tests/test_csg_certain_host.py,
# scripts/csg_certain_census.py) and of the planner's kCsgCertain flag (tests/test_csg_certain_plan.py), without ROCm
tests/libcsg_certain_check.so: tests/csg_certain_check.cpp $(CSRC)/csg_certain.h $(CSRC)/scene_plan.cpp $(CSRC)/scene_plan.h $(CSRC)/c2rt_device.h $(CSRC)/csg_void.h $(CSRC)/ground_certain.h include/c2rt.h
	g++ -O2 -std=c++17 -fPIC -shared $(FPFLAGS) -Wall -o $@ tests/csg_certain_check.cpp $(CSRC)/scene_plan.cpp

# host build of the planner's decision which nodes a frame may render beside the ground through lean::csg_tile
# (tests/test_csg_tile_plan.py, tests/test_gpu_csg_tiles.py, scripts/csg_tile_census.py), without ROCm
tests/libcsg_tile_check.so: tests/csg_tile_check.cpp $(CSRC)/scene_plan.cpp $(CSRC)/scene_plan.h $(CSRC)/c2rt_device.h $(CSRC)/csg_void.h $(CSRC)/ground_certain.h include/c2rt.h
	g++ -O2 -std=c++17 -fPIC -shared $(FPFLAGS) -Wall -o $@ tests/csg_tile_check.cpp $(CSRC)/scene_plan.cpp

# host build of the sphere-silhouette test of the mask pre-pass (tests/test_sphere_cull_tiles.py, scripts/sphere_cull_tiles.py)
tests/libsphere_cull_check.so: tests/sphere_cull_check.cpp $(CSRC)/csg_void.h
	g++ -O2 -std=c++17 -fPIC -shared $(FPFLAGS) -Wall -o $@ $<

# host build of the planner, without ROCm on the include path: the build itself enforces that scene_plan.cpp is HIP-free
# (tests/test_scene_plan.py holds it to the restatements in scripts/csg_void_tiles.py and scripts/sphere_cull_tiles.py)
tests/libscene_plan_check.so: tests/scene_plan_check.cpp $(CSRC)/scene_plan.cpp $(CSRC)/scene_plan.h $(CSRC)/c2rt_device.h $(CSRC)/csg_void.h $(CSRC)/ground_certain.h include/c2rt.h
	g++ -O2 -std=c++17 -fPIC -shared $(FPFLAGS) -Wall -o $@ tests/scene_plan_check.cpp $(CSRC)/scene_plan.cpp

# host build of the pose-and-replan step behind c2rt_update_scene and c2rt_render_frames_posed (tests/test_scene_update_plan.py),
# without ROCm like the planner's: what it drives is scene_plan.cpp's own update_scene_plan, not a copy of it
tests/libscene_update_check.so: tests/scene_update_check.cpp $(CSRC)/scene_plan.cpp $(CSRC)/scene_plan.h $(CSRC)/c2rt_device.h $(CSRC)/csg_void.h $(CSRC)/ground_certain.h include/c2rt.h
	g++ -O2 -std=c++17 -fPIC -shared $(FPFLAGS) -Wall -o $@ tests/scene_update_check.cpp $(CSRC)/scene_plan.cpp

# host build of the planner's decision which frames take the ground-tile path (tests/test_ground_fast_plan.py), without ROCm
tests/libground_fast_check.so: tests/ground_fast_check.cpp $(CSRC)/scene_plan.cpp $(CSRC)/scene_plan.h $(CSRC)/c2rt_device.h $(CSRC)/csg_void.h $(CSRC)/ground_certain.h include/c2rt.h
	g++ -O2 -std=c++17 -fPIC -shared $(FPFLAGS) -Wall -o $@ tests/ground_fast_check.cpp $(CSRC)/scene_plan.cpp

# host build of the dark-tile test of the mask pre-pass and of the planner's part of it (tests/test_ground_dark_tiles.py,
# scripts/ground_dark_tiles.py), without ROCm
tests/libground_dark_check.so: tests/ground_dark_check.cpp $(CSRC)/scene_plan.cpp $(CSRC)/scene_plan.h $(CSRC)/c2rt_device.h $(CSRC)/csg_void.h $(CSRC)/ground_certain.h include/c2rt.h
	g++ -O2 -std=c++17 -fPIC -shared $(FPFLAGS) -Wall -o $@ tests/ground_dark_check.cpp $(CSRC)/scene_plan.cpp

# host build of the sphere-interior test of the mask pre-pass and of the planner's part of it (tests/test_sphere_interior_tiles.py,
# tests/test_gpu_sphere_tiles.py, scripts/sphere_interior_tiles.py), without ROCm
tests/libsphere_interior_check.so: tests/sphere_interior_check.cpp $(CSRC)/scene_plan.cpp $(CSRC)/scene_plan.h $(CSRC)/c2rt_device.h $(CSRC)/csg_void.h $(CSRC)/ground_certain.h include/c2rt.h
	g++ -O2 -std=c++17 -fPIC -shared $(FPFLAGS) -Wall -o $@ tests/sphere_interior_check.cpp $(CSRC)/scene_plan.cpp

# host build of the planner's decision which frames take the short chain for ground tiles (tests/test_ground_certain_plan.py), without ROCm
tests/libground_certain_check.so: tests/ground_certain_plan_check.cpp $(CSRC)/scene_plan.cpp $(CSRC)/scene_plan.h $(CSRC)/c2rt_device.h $(CSRC)/csg_void.h $(CSRC)/ground_certain.h include/c2rt.h
	g++ -O2 -std=c++17 -fPIC -shared $(FPFLAGS) -Wall -o $@ tests/ground_certain_plan_check.cpp $(CSRC)/scene_plan.cpp

# host build of the planner's two decisions behind the short chain's texel fetch and light term (tests/test_ground_texel_plan.py), without ROCm
tests/libground_texel_check.so: tests/ground_texel_plan_check.cpp $(CSRC)/scene_plan.cpp $(CSRC)/scene_plan.h $(CSRC)/c2rt_device.h $(CSRC)/csg_void.h $(CSRC)/ground_certain.h include/c2rt.h
	g++ -O2 -std=c++17 -fPIC -shared $(FPFLAGS) -Wall -o $@ tests/ground_texel_plan_check.cpp $(CSRC)/scene_plan.cpp

# device check of the short chain's tap average and texel blend against the compiler's division and bitmap_filtered
# (tests/test_gpu_tap_average.py runs it)
tests/tap_average_check: tests/tap_average_check.hip $(TRACE_DEPS)
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 $(FPFLAGS) -fhip-fp32-correctly-rounded-divide-sqrt $< -o $@

# host check of ground_certain.h against the reference's chain in IEEE doubles (tests/test_ground_certain_host.py builds
# its own copy; `make tests/ground_certain_check SAN=-fsanitize=address,undefined` for a sanitizer run of the same program)
tests/ground_certain_check: tests/ground_certain_check.c $(CSRC)/ground_certain.h
	$(CC) -O2 -std=gnu11 $(FPFLAGS) -fopenmp -Wall $(SAN) -o $@ $< -lm

# CPU oracle: plain C restatement of the reference algorithm (tests only)
oracle/libc2rt_oracle.so: oracle/c2rt_oracle.c oracle/c2rt_oracle.h include/c2rt.h
	$(CC) -O2 -std=gnu11 -fPIC -shared $(FPFLAGS) -Wall -o $@ oracle/c2rt_oracle.c -lm -lpthread

# the same restatement with its arithmetic statements tallied (algorithmic fp op count for bench.py's roofline.flops)
oracle/libc2rt_oracle_count.so: oracle/c2rt_oracle.c oracle/c2rt_oracle.h include/c2rt.h
	$(CC) -O2 -std=gnu11 -fPIC -shared $(FPFLAGS) -Wall -DORC_COUNT_OPS -o $@ oracle/c2rt_oracle.c -lm -lpthread

# the compiler's own per-kernel register / scratch / occupancy figures (committed as profiles/rNN_resource_usage.txt:
# rocprofv3's VGPR_Count column is in allocation granules and does not show them)
resource-usage: | $(BUILD)
	@$(foreach u,$(UNITS),$(HIPCC) $(HIPFLAGS) $(KERNELFLAGS) $(KERNELFLAGS_u$(u)) $(EXTRA_KERNEL_FLAGS) -DC2RT_UNIT=$(u) -Rpass-analysis=kernel-resource-usage \
	    -c $(CSRC)/c2rt_kernels.hip -o $(BUILD)/ru_u$(u).o 2>&1 | grep -E "remark:" | sed -e 's/.*remark: [^ ]* *//' -e 's/ \[-Rpass-analysis=kernel-resource-usage\]//' ;)
	@$(foreach q,$(QUERIES),$(HIPCC) $(HIPFLAGS) $(KERNELFLAGS) $(KERNELFLAGS_QUERY) $(EXTRA_KERNEL_FLAGS) -Rpass-analysis=kernel-resource-usage \
	    -c $(CSRC)/$(q).hip -o $(BUILD)/ru_$(q).o 2>&1 | grep -E "remark:" | sed -e 's/.*remark: [^ ]* *//' -e 's/ \[-Rpass-analysis=kernel-resource-usage\]//' ;)

clean:
	rm -rf build build_* chess2rt_amd/libc2rt*.so oracle/libc2rt_oracle.so oracle/libc2rt_oracle_count.so tests/fp64_lean_check tests/certain_f32_check tests/libcsg_void_check.so tests/libsphere_cull_check.so tests/libscene_plan_check.so tests/libscene_update_check.so tests/libground_fast_check.so tests/libground_dark_check.so tests/libground_certain_check.so tests/ground_certain_check tests/libground_texel_check.so tests/libsphere_interior_check.so tests/libcsg_certain_check.so tests/libcsg_tile_check.so tests/tap_average_check

.PHONY: all clean resource-usage
