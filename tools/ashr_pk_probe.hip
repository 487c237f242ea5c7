// ashr_pk_probe.hip -- does gfx950's v_ashr_pk_u8_i32 write the upper 16 bits of its destination?
// One wave; the destination register holds 0xdeadbeef before the instruction.
//     hipcc --offload-arch=gfx950 -O2 -o ashr_pk_probe tools/ashr_pk_probe.hip && ./ashr_pk_probe
// MI355X answers 0xdeadff64 (profiles/ashr_pk_probe.txt): the two saturated bytes, the upper half KEPT.
// hipcc treats that half as zero when it ORs the next pair of bytes in above it, which is why
// k_output_rgb clamps before it shifts (k_output.hip: rgb_clip255_sh17, tests/test_isa_output_rgb.py).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
__global__ void probe(uint32_t* out, int a, int b, int sh)
{
    uint32_t d = 0xdeadbeefu;
    int va = a + (int)threadIdx.x, vb = b - (int)threadIdx.x, vs = sh;
    asm volatile("v_ashr_pk_u8_i32 %0, %1, %2, %3" : "+v"(d) : "v"(va), "v"(vb), "v"(vs));
    out[threadIdx.x] = d;
}
int main()
{
    uint32_t* d; uint32_t h[64];
    if (hipMalloc(&d, sizeof h) != hipSuccess) return 2;
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, d, 100 << 17, 300 << 17, 17);
    if (hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return 3;
    for (int i = 0; i < 4; ++i) printf("lane %d: 0x%08x\n", i, h[i]);
    printf("upper half %s\n", (h[0] >> 16) == 0xdead ? "KEPT (not written)" : (h[0] >> 16) == 0 ? "zeroed" : "other");
    return 0;
}
