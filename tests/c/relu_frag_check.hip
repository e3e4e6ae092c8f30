// relu_frag_check.hip -- tests/test_gpu_relu_frag.py builds this into a small shared object of its own.
// Every lane takes 16 float32 values as an activation tensor (four accumulator tiles) and writes the operand
// fragments of relu(x) in both forms of encoder_core.h: split_act(relu4(x)), and relu_frag(split_act(x)).
#include "encoder_core.h"

namespace {
__global__ void frag_kernel(const float* __restrict__ x, uint32_t* __restrict__ ref, uint32_t* __restrict__ got, int n16) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n16) return;
    qb::f32x4 in[4], rl[4];
    for (int m = 0; m < 4; ++m) {
        in[m] = qb::load4(x + 16 * i + 4 * m);
        rl[m] = qb::relu4(in[m]);
    }
    const qb::ActFrag a = qb::split_act<false>(rl);
    const qb::ActFrag b = qb::relu_frag(qb::split_act<false>(in));
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    auto put = [&](uint32_t* out, const qb::ActFrag& f) {
        for (int s = 0; s < 2; ++s) {
            const u32x4 h = __builtin_bit_cast(u32x4, f.hi[s]), l = __builtin_bit_cast(u32x4, f.lo[s]);
            for (int p = 0; p < 4; ++p) {
                out[16 * i + 8 * s + p] = h[p];       // halves of values 8 s + 2 p, 8 s + 2 p + 1
                out[16 * i + 8 * s + 4 + p] = l[p];
            }
        }
    };
    put(ref, a);
    put(got, b);
}
}  // namespace

// x: n16 * 16 host floats; ref, got: n16 * 16 host dwords.  Returns 0, or the HIP error code.
extern "C" int relu_frag_check(const float* x, int n16, uint32_t* ref, uint32_t* got) {
    const size_t bytes = (size_t)n16 * 16 * 4;
    float* dx = nullptr;
    uint32_t *dr = nullptr, *dg = nullptr;
    hipError_t e;
    if ((e = hipMalloc(&dx, bytes)) != hipSuccess) return (int)e;
    if ((e = hipMalloc(&dr, bytes)) != hipSuccess) return (int)e;
    if ((e = hipMalloc(&dg, bytes)) != hipSuccess) return (int)e;
    if ((e = hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(frag_kernel, dim3((n16 + 255) / 256), dim3(256), 0, 0, dx, dr, dg, n16);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if ((e = hipMemcpy(ref, dr, bytes, hipMemcpyDeviceToHost)) != hipSuccess) return (int)e;
    if ((e = hipMemcpy(got, dg, bytes, hipMemcpyDeviceToHost)) != hipSuccess) return (int)e;
    (void)hipFree(dx);
    (void)hipFree(dr);
    (void)hipFree(dg);
    return 0;
}
