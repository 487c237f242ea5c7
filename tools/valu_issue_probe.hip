// tools/valu_issue_probe.hip -- issue cost of the vector instructions k_inter4r is made of, at the
// kernel's own occupancy (5 waves per SIMD, 256-thread workgroups, every CU busy): each kernel runs
// one instruction ITER x 16 times per wave on eight independent registers, and the host prints the
// time per wave-instruction relative to v_fma_f32.  DESIGN.md section 3 quotes the table.
//   hipcc --offload-arch=gfx950 -O3 tools/valu_issue_probe.hip -o valu_issue_probe && ./valu_issue_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define ITER 2048
#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

typedef float f32x2 __attribute__((ext_vector_type(2)));

// 16 instructions on registers a0..a7 (32-bit) / p0..p7 (64-bit pairs), twice round
#define R8(OP) OP(0) OP(1) OP(2) OP(3) OP(4) OP(5) OP(6) OP(7)
#define KERNEL32(NAME, ASM)                                                                                   \
    __global__ __launch_bounds__(256, 5) void NAME(uint32_t* out, uint32_t x, uint32_t y)                      \
    {                                                                                                         \
        uint32_t a[8], b = x + threadIdx.x, c = y ^ threadIdx.x;                                              \
        const uint64_t m = ((uint64_t)x << 32) | y;           /* a lane mask in an SGPR pair */                 \
        for (int k = 0; k < 8; ++k) a[k] = x * (k + 1) + threadIdx.x;                                         \
        for (int i = 0; i < ITER; ++i) {                                                                      \
            _Pragma("unroll") for (int k = 0; k < 8; ++k) asm volatile(ASM : "+v"(a[k]) : "v"(b), "v"(c), "s"(m) : "vcc"); \
            _Pragma("unroll") for (int k = 0; k < 8; ++k) asm volatile(ASM : "+v"(a[k]) : "v"(b), "v"(c), "s"(m) : "vcc"); \
        }                                                                                                     \
        uint32_t s = 0;                                                                                       \
        for (int k = 0; k < 8; ++k) s ^= a[k];                                                                \
        if (s == 0x12345678u) out[threadIdx.x] = s;                                                           \
    }
#define KERNEL64(NAME, ASM)                                                                                   \
    __global__ __launch_bounds__(256, 5) void NAME(uint32_t* out, uint32_t x, uint32_t y)                      \
    {                                                                                                         \
        uint64_t a[8], b = ((uint64_t)x << 32) | threadIdx.x, c = ((uint64_t)y << 32) ^ threadIdx.x;          \
        const uint32_t b32 = x + threadIdx.x, c32 = y ^ threadIdx.x;                                          \
        for (int k = 0; k < 8; ++k) a[k] = (uint64_t)x * (k + 1) + threadIdx.x;                               \
        for (int i = 0; i < ITER; ++i) {                                                                      \
            _Pragma("unroll") for (int k = 0; k < 8; ++k) asm volatile(ASM : "+v"(a[k]) : "v"(b), "v"(c), "v"(b32), "v"(c32) : "vcc"); \
            _Pragma("unroll") for (int k = 0; k < 8; ++k) asm volatile(ASM : "+v"(a[k]) : "v"(b), "v"(c), "v"(b32), "v"(c32) : "vcc"); \
        }                                                                                                     \
        uint64_t s = 0;                                                                                       \
        for (int k = 0; k < 8; ++k) s ^= a[k];                                                                \
        if (s == 0x12345678u) out[threadIdx.x] = (uint32_t)s;                                                 \
    }

// a 64-bit accumulator as two halves plus a temporary, for the sequences that replace one 64-bit instruction
#define KERNEL64S(NAME, ASM)                                                                                  \
    __global__ __launch_bounds__(256, 5) void NAME(uint32_t* out, uint32_t x, uint32_t y)                      \
    {                                                                                                         \
        uint32_t lo[8], hi[8], t[8], b = x + threadIdx.x, c = y ^ threadIdx.x;                                \
        for (int k = 0; k < 8; ++k) { lo[k] = x * (k + 1) + threadIdx.x; hi[k] = y + k; t[k] = k; }           \
        for (int i = 0; i < ITER; ++i) {                                                                      \
            _Pragma("unroll") for (int k = 0; k < 8; ++k) asm volatile(ASM : "+v"(lo[k]), "+v"(hi[k]), "+v"(t[k]) : "v"(b), "v"(c) : "vcc"); \
            _Pragma("unroll") for (int k = 0; k < 8; ++k) asm volatile(ASM : "+v"(lo[k]), "+v"(hi[k]), "+v"(t[k]) : "v"(b), "v"(c) : "vcc"); \
        }                                                                                                     \
        uint32_t s = 0;                                                                                       \
        for (int k = 0; k < 8; ++k) s ^= lo[k] ^ hi[k] ^ t[k];                                                \
        if (s == 0x12345678u) out[threadIdx.x] = s;                                                           \
    }

KERNEL32(k_fma_f32, "v_fma_f32 %0, %0, %1, %2")
KERNEL32(k_add_u32, "v_add_u32 %0, %0, %1")
KERNEL32(k_pk_add_u16, "v_pk_add_u16 %0, %0, %1")
KERNEL32(k_pk_mad_u16, "v_pk_mad_u16 %0, %0, %1, %2")
KERNEL32(k_pk_max_i16, "v_pk_max_i16 %0, %0, %1")
KERNEL32(k_pk_ashr_i16, "v_pk_ashrrev_i16 %0, 1, %0")
KERNEL32(k_perm_b32, "v_perm_b32 %0, %0, %1, %2")
KERNEL32(k_alignbyte, "v_alignbyte_b32 %0, %0, %1, %2")
KERNEL32(k_cndmask, "v_cndmask_b32 %0, %0, %1, vcc")
KERNEL32(k_cndmask_sgpr, "v_cndmask_b32_e64 %0, %0, %1, %3")
KERNEL32(k_add_u32_e64, "v_add_u32_e64 %0, %0, %1")
KERNEL32(k_add3_u32, "v_add3_u32 %0, %0, %1, %2")
KERNEL32(k_and_b32, "v_and_b32 %0, %0, %1")
KERNEL32(k_max_i32, "v_max_i32 %0, %0, %1")
KERNEL32(k_lshlrev_b32, "v_lshlrev_b32 %0, 1, %0")
KERNEL32(k_bitop3, "v_bitop3_b32 %0, %0, %1, %2 bitop3:0xe4")
KERNEL32(k_cmp_cndmask, "v_cmp_lt_i32 vcc, %0, %1\n v_cndmask_b32 %0, %0, %1, vcc")
KERNEL32(k_bfi_b32, "v_bfi_b32 %0, %0, %1, %2")
KERNEL32(k_med3_f32, "v_med3_f32 %0, %0, %1, %2")
KERNEL32(k_med3_i32, "v_med3_i32 %0, %0, %1, %2")
KERNEL32(k_cvt_i32_f32, "v_cvt_i32_f32 %0, %0")
KERNEL32(k_cvt_f32_i32_sdwa, "v_cvt_f32_i32_sdwa %0, sext(%0) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1")
KERNEL32(k_dot2_i32_i16, "v_dot2_i32_i16 %0, %1, %2, %0")
KERNEL32(k_mad_u32_u24, "v_mad_u32_u24 %0, %0, %1, %2")
KERNEL32(k_mad_i32_i24, "v_mad_i32_i24 %0, %0, %1, %2")
KERNEL32(k_mul_lo_u32, "v_mul_lo_u32 %0, %0, %1")
KERNEL32(k_sad_u32, "v_sad_u32 %0, %0, %1, %2")
KERNEL32(k_lshl_or_b32, "v_lshl_or_b32 %0, %0, 16, %1")
KERNEL32(k_mov_dpp, "v_mov_b32_dpp %0, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf")
KERNEL64(k_pk_fma_f32, "v_pk_fma_f32 %0, %0, %1, %2")
KERNEL64(k_pk_add_f32, "v_pk_add_f32 %0, %0, %1")
KERNEL64(k_mad_i64_i32, "v_mad_i64_i32 %0, vcc, %3, %4, %0")
KERNEL64(k_lshl_add_u64, "v_lshl_add_u64 %0, %0, 0, %1")
// what would replace v_mad_i64_i32 in an address: a 24-bit product added to a 64-bit base (three instructions per slot)
KERNEL64S(k_mul_u24_add_u64, "v_mul_u32_u24 %2, %3, %4\n v_add_co_u32 %0, vcc, %0, %2\n v_addc_co_u32 %1, vcc, 0, %1, vcc")

struct Probe {
    const char* name;
    void (*fn)(uint32_t*, uint32_t, uint32_t);
};
#define P(n) {#n, n}

int main()
{
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    uint32_t* out;
    CHECK(hipMalloc(&out, 4096));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    const Probe probes[] = {P(k_fma_f32), P(k_add_u32), P(k_pk_add_u16), P(k_pk_mad_u16), P(k_pk_max_i16), P(k_pk_ashr_i16),
                            P(k_perm_b32), P(k_alignbyte), P(k_cndmask), P(k_cndmask_sgpr), P(k_add_u32_e64), P(k_add3_u32), P(k_and_b32),
                            P(k_max_i32), P(k_lshlrev_b32), P(k_bitop3), P(k_cmp_cndmask), P(k_bfi_b32), P(k_med3_f32), P(k_med3_i32),
                            P(k_cvt_i32_f32), P(k_cvt_f32_i32_sdwa), P(k_dot2_i32_i16), P(k_mad_u32_u24), P(k_mad_i32_i24),
                            P(k_mul_lo_u32), P(k_sad_u32), P(k_lshl_or_b32), P(k_mov_dpp), P(k_pk_fma_f32), P(k_pk_add_f32),
                            P(k_mad_i64_i32), P(k_lshl_add_u64), P(k_mul_u24_add_u64)};
    // 5 workgroups of 4 waves per CU: 5 waves per SIMD, three rounds of them
    const dim3 grid(cus * 5 * 3), block(256);
    double base = 0;
    for (const Probe& p : probes) {
        float best = 1e30f;
        for (int rep = 0; rep < 4; ++rep) {
            CHECK(hipEventRecord(e0));
            hipLaunchKernelGGL(p.fn, grid, block, 0, 0, out, 3u, 5u);
            CHECK(hipEventRecord(e1));
            CHECK(hipEventSynchronize(e1));
            float ms;
            CHECK(hipEventElapsedTime(&ms, e0, e1));
            if (rep && ms < best) best = ms;
        }
        CHECK(hipGetLastError());
        // wave-instructions per SIMD: 15 waves x ITER x 16
        const double ns = best * 1e6 / (15.0 * ITER * 16);
        if (base == 0) base = ns;
        printf("%-22s %8.3f ms  %6.3f ns per wave-instruction per SIMD  x%.2f of v_fma_f32\n", p.name, best, ns, ns / base);
    }
    return 0;
}
