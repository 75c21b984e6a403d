// Which roundings does torch's device lerp take on this GPU?  The four candidate forms of the statement in ATen/native/Lerp.h
// (d = p - a; |w| < 0.5 ? a + w * d : p - d * (1 - w)): bit 0 of `form` fuses the product and the sum of the first branch, bit 1 those
// of the second.  tools/lerp_form_probe.py runs them against torch._foreach_lerp_ / torch.lerp and counts differing elements.
// Build WITH contraction off -- `__fmul_rn` / `__fadd_rn` / `__fsub_rn` are plain operators in this HIP, and the default setting
// fuses all four forms into the same code:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared lerp_form_probe.hip -o liblerp_form_probe.so
#include <hip/hip_runtime.h>

template <int FORM>
__global__ void lerp_form_kernel(float* a, const float* p, long long n, float w) {
    const float omw = __fsub_rn(1.f, w);
    const bool small = fabsf(w) < 0.5f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float av = a[i], pv = p[i];
        const float d = __fsub_rn(pv, av);
        float r;
        if (small) r = (FORM & 1) ? __fmaf_rn(w, d, av) : __fadd_rn(av, __fmul_rn(w, d));
        else r = (FORM & 2) ? __fmaf_rn(-d, omw, pv) : __fsub_rn(pv, __fmul_rn(d, omw));
        a[i] = r;
    }
}

extern "C" int probe_lerp(float* a, const float* p, long long n, float w, int form, void* stream) {
    if (n <= 0 || !a || !p || form < 0 || form > 3) return -1;
    int g = (int)((n + 255) / 256);
    if (g > 2048) g = 2048;
    switch (form) {
        case 0: hipLaunchKernelGGL(lerp_form_kernel<0>, dim3(g), dim3(256), 0, (hipStream_t)stream, a, p, n, w); break;
        case 1: hipLaunchKernelGGL(lerp_form_kernel<1>, dim3(g), dim3(256), 0, (hipStream_t)stream, a, p, n, w); break;
        case 2: hipLaunchKernelGGL(lerp_form_kernel<2>, dim3(g), dim3(256), 0, (hipStream_t)stream, a, p, n, w); break;
        default: hipLaunchKernelGGL(lerp_form_kernel<3>, dim3(g), dim3(256), 0, (hipStream_t)stream, a, p, n, w); break;
    }
    return (int)hipGetLastError();
}
