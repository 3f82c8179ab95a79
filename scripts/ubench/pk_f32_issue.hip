// Issue cost (cycles per wave-instruction) of the fp32 / integer VALU instructions a texel fetch and blend is made of:
// single against packed fp32 (also with an op_sel broadcast operand and with the register shuffles the SLP vectoriser
// puts around them), the 32-bit against the 24-bit multiply, 64-bit against 32-bit address arithmetic — independent
// streams, on one SIMD with 1 and 4 resident waves.  Modelled on fp64_issue.hip.
// Build: hipcc --offload-arch=gfx950 -O2 pk_f32_issue.hip -o pk_f32_issue
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>

#define REP8(x) x x x x x x x x

// d0..d3: four independent 64-bit destinations (register pairs); a, b, c: 64-bit sources; the 32-bit forms use
// f0..f3 / i0..i3 and fa, fb, fc / ia, ib.  Four instructions per body, 32 per loop trip.
#define KERNEL(name, body)                                                                                      \
    __global__ void __launch_bounds__(1024) name(unsigned long long *out, int iters, double seed)                \
    {                                                                                                           \
        double a = seed + threadIdx.x, b = seed * 3 + 1, c = 1.5, d0, d1, d2, d3;                               \
        d0 = d1 = d2 = d3 = a;                                                                                  \
        float fa = (float)a, fb = 2.0f, fc = 0.5f, f0 = 1.0f, f1 = 1.0f, f2 = 1.0f, f3 = 1.0f;                  \
        unsigned ia = threadIdx.x, ib = 3, i0 = 0, i1 = 0, i2 = 0, i3 = 0;                                      \
        unsigned long long t0 = __builtin_amdgcn_s_memtime();                                                   \
        for (int i = 0; i < iters; ++i) {                                                                       \
            REP8(body)                                                                                          \
        }                                                                                                       \
        unsigned long long t1 = __builtin_amdgcn_s_memtime();                                                   \
        if (d0 + d1 + d2 + d3 + f0 + f1 + f2 + f3 + i0 + i1 + i2 + i3 == 12345.678) out[1000] = 1;              \
        if ((threadIdx.x & 63) == 0) out[blockIdx.x * 16 + threadIdx.x / 64] = t1 - t0;                         \
    }

#define F2(ins) asm volatile(ins " %0, %4, %5\n" ins " %1, %4, %5\n" ins " %2, %4, %5\n" ins " %3, %4, %5" \
                             : "+v"(f0), "+v"(f1), "+v"(f2), "+v"(f3) : "v"(fa), "v"(fb));
#define F3(ins) asm volatile(ins " %0, %4, %5, %6\n" ins " %1, %4, %5, %6\n" ins " %2, %4, %5, %6\n" ins " %3, %4, %5, %6" \
                             : "+v"(f0), "+v"(f1), "+v"(f2), "+v"(f3) : "v"(fa), "v"(fb), "v"(fc));
#define F1(ins) asm volatile(ins " %0, %4\n" ins " %1, %4\n" ins " %2, %4\n" ins " %3, %4" \
                             : "+v"(f0), "+v"(f1), "+v"(f2), "+v"(f3) : "v"(fa));
#define P2(ins, mods) asm volatile(ins " %0, %4, %5" mods "\n" ins " %1, %4, %5" mods "\n" ins " %2, %4, %5" mods "\n" ins " %3, %4, %5" mods \
                             : "+v"(d0), "+v"(d1), "+v"(d2), "+v"(d3) : "v"(a), "v"(b));
#define P3(ins, mods) asm volatile(ins " %0, %4, %5, %6" mods "\n" ins " %1, %4, %5, %6" mods "\n" ins " %2, %4, %5, %6" mods "\n" ins " %3, %4, %5, %6" mods \
                             : "+v"(d0), "+v"(d1), "+v"(d2), "+v"(d3) : "v"(a), "v"(b), "v"(c));
#define I2(ins) asm volatile(ins " %0, %4, %5\n" ins " %1, %4, %5\n" ins " %2, %4, %5\n" ins " %3, %4, %5" \
                             : "+v"(i0), "+v"(i1), "+v"(i2), "+v"(i3) : "v"(ia), "v"(ib));
#define I3(ins) asm volatile(ins " %0, %4, %5, %4\n" ins " %1, %4, %5, %4\n" ins " %2, %4, %5, %4\n" ins " %3, %4, %5, %4" \
                             : "+v"(i0), "+v"(i1), "+v"(i2), "+v"(i3) : "v"(ia), "v"(ib));
#define I3SH(ins) asm volatile(ins " %0, %4, 4, %5\n" ins " %1, %4, 4, %5\n" ins " %2, %4, 4, %5\n" ins " %3, %4, 4, %5" \
                             : "+v"(i0), "+v"(i1), "+v"(i2), "+v"(i3) : "v"(ia), "v"(ib));
#define I3ADDSH(ins) asm volatile(ins " %0, %4, %5, 4\n" ins " %1, %4, %5, 4\n" ins " %2, %4, %5, 4\n" ins " %3, %4, %5, 4" \
                             : "+v"(i0), "+v"(i1), "+v"(i2), "+v"(i3) : "v"(ia), "v"(ib));
#define MAD64 asm volatile("v_mad_u64_u32 %0, vcc, %4, %5, %6\nv_mad_u64_u32 %1, vcc, %4, %5, %6\nv_mad_u64_u32 %2, vcc, %4, %5, %6\nv_mad_u64_u32 %3, vcc, %4, %5, %6" \
                             : "+v"(d0), "+v"(d1), "+v"(d2), "+v"(d3) : "v"(ia), "v"(ib), "v"(a) : "vcc");
#define LSHLADD64 asm volatile("v_lshl_add_u64 %0, %4, 4, %5\nv_lshl_add_u64 %1, %4, 4, %5\nv_lshl_add_u64 %2, %4, 4, %5\nv_lshl_add_u64 %3, %4, 4, %5" \
                             : "+v"(d0), "+v"(d1), "+v"(d2), "+v"(d3) : "v"(a), "v"(b));
#define LSHL64 asm volatile("v_lshlrev_b64 %0, 4, %4\nv_lshlrev_b64 %1, 4, %4\nv_lshlrev_b64 %2, 4, %4\nv_lshlrev_b64 %3, 4, %4" \
                             : "+v"(d0), "+v"(d1), "+v"(d2), "+v"(d3) : "v"(a));
#define PKMOV asm volatile("v_pk_mov_b32 %0, %4, %5 op_sel:[1,0]\nv_pk_mov_b32 %1, %4, %5 op_sel:[1,0]\nv_pk_mov_b32 %2, %4, %5 op_sel:[1,0]\nv_pk_mov_b32 %3, %4, %5 op_sel:[1,0]" \
                             : "+v"(d0), "+v"(d1), "+v"(d2), "+v"(d3) : "v"(a), "v"(b));
// what the frame kernel's blend is made of, per two channels of one texel: a packed product behind one shuffle move
// against two single products
#define PKMUL_MOV asm volatile("v_mov_b32 %2, %4\nv_pk_mul_f32 %0, %5, %6\nv_mov_b32 %3, %4\nv_pk_mul_f32 %1, %5, %6" \
                             : "+v"(d0), "+v"(d1), "+v"(f0), "+v"(f1) : "v"(fa), "v"(a), "v"(b));

KERNEL(k_mul, F2("v_mul_f32"))
KERNEL(k_add, F2("v_add_f32"))
KERNEL(k_fma, F3("v_fma_f32"))
KERNEL(k_mov, F1("v_mov_b32"))
KERNEL(k_pk_mul, P2("v_pk_mul_f32", ""))
KERNEL(k_pk_add, P2("v_pk_add_f32", ""))
KERNEL(k_pk_fma, P3("v_pk_fma_f32", ""))
KERNEL(k_pk_mul_b, P2("v_pk_mul_f32", " op_sel_hi:[1,0]"))
KERNEL(k_pk_add_b, P2("v_pk_add_f32", " op_sel_hi:[1,0]"))
KERNEL(k_pk_fma_b, P3("v_pk_fma_f32", " op_sel_hi:[1,0,1]"))
KERNEL(k_pk_mov, PKMOV)
KERNEL(k_pk_mul_mov, PKMUL_MOV)
KERNEL(k_mul_lo, I2("v_mul_lo_u32"))
KERNEL(k_mul_u24, I2("v_mul_u32_u24"))
KERNEL(k_mad_u24, I3("v_mad_u32_u24"))
KERNEL(k_mad64, MAD64)
KERNEL(k_lshl_add64, LSHLADD64)
KERNEL(k_lshl64, LSHL64)
KERNEL(k_lshl_add32, I3SH("v_lshl_add_u32"))
KERNEL(k_add_lshl32, I3ADDSH("v_add_lshl_u32"))
KERNEL(k_add32, I2("v_add_u32"))

typedef void (*kern_t)(unsigned long long *, int, double);
struct Entry { const char *name; kern_t k; };

#define CHECK(x)                                                                               \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                            \
            return 1;                                                                          \
        }                                                                                      \
    } while (0)

int main()
{
    Entry es[] = {{"v_add_f32", k_add}, {"v_mul_f32", k_mul}, {"v_fma_f32", k_fma}, {"v_mov_b32", k_mov},
                  {"v_pk_mul_f32", k_pk_mul}, {"v_pk_add_f32", k_pk_add}, {"v_pk_fma_f32", k_pk_fma},
                  {"v_pk_mul_f32 bcast", k_pk_mul_b}, {"v_pk_add_f32 bcast", k_pk_add_b}, {"v_pk_fma_f32 bcast", k_pk_fma_b},
                  {"v_pk_mov_b32", k_pk_mov}, {"v_mov+v_pk_mul pairs", k_pk_mul_mov},
                  {"v_mul_lo_u32", k_mul_lo}, {"v_mul_u32_u24", k_mul_u24}, {"v_mad_u32_u24", k_mad_u24},
                  {"v_mad_u64_u32", k_mad64}, {"v_lshl_add_u64", k_lshl_add64}, {"v_lshlrev_b64", k_lshl64},
                  {"v_lshl_add_u32", k_lshl_add32}, {"v_add_lshl_u32", k_add_lshl32}, {"v_add_u32", k_add32}};
    unsigned long long *out;
    // 256 blocks x 16 waves of time stamps, and the word at index 1000 the kernels never write
    CHECK(hipMalloc(&out, 8192 * 8));
    const int iters = 100000;
    // warm the clocks
    for (int i = 0; i < 20; ++i) hipLaunchKernelGGL(k_fma, dim3(256), dim3(1024), 0, 0, out, iters / 10, 1.0);
    CHECK(hipDeviceSynchronize());
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    printf("%-22s %9s %9s   ns per wave-instruction with 1 / 4 waves on each SIMD of one CU (x2.4 = cycles at 2.4 GHz); last: ratio to v_add_f32 at 4 waves\n", "instruction", "1 wave", "4 waves");
    double ref = 0;
    for (int pass = 0; pass < 2; ++pass)
        for (auto &e : es) {
            double res[2];
            const int wv[2] = {1, 4};
            for (int w = 0; w < 2; ++w) {
                const int threads = 64 * 4 * wv[w];
                // every CU busy (256 blocks) so that the chip sits at its loaded clock
                hipLaunchKernelGGL(e.k, dim3(256), dim3(threads), 0, 0, out, iters / 20, 1.0);
                CHECK(hipEventRecord(e0));
                hipLaunchKernelGGL(e.k, dim3(256), dim3(threads), 0, 0, out, iters, 1.0);
                CHECK(hipEventRecord(e1));
                CHECK(hipDeviceSynchronize());
                float ms = 0;
                CHECK(hipEventElapsedTime(&ms, e0, e1));
                // per SIMD: wv waves x iters x 32 instructions in ms
                res[w] = (double)ms * 1e6 / ((double)iters * 32.0 * wv[w]);
            }
            if (pass == 0) {
                if (!strcmp(e.name, "v_add_f32")) ref = res[1];
                continue;
            }
            printf("%-22s %9.3f %9.3f   cycles@2.4: %6.2f %6.2f   x%.2f\n", e.name, res[0], res[1], res[0] * 2.4, res[1] * 2.4, res[1] / ref);
        }
    CHECK(hipFree(out));
    return 0;
}
