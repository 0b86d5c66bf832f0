// Diagnostic measurement (not part of the product): the absolute error of the log objective's map ln(m + floor) as the
// spectral kernels compute it (obj_ln_floor, csrc/kernels/objective.h: v_log_f32 of the fp32 sum, times ln 2 in fp32)
// against libm's fp64 log of the exact sum, for magnitudes m in [0, 2 - floor] - arguments in [floor, 2].  The expression
// below is that routine's, compiled with the library's -ffp-contract=off.  Every `stride`-th fp32 value of the range is
// visited; the maximum is reported per floor, with the argument it occurred at.  DESIGN.md 4.6 quotes the result.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o ln_map_error ln_map_error.hip && ./ln_map_error [stride]
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

__global__ __launch_bounds__(256) void k_map(float *out, uint32_t first_bits, uint32_t stride, uint32_t n, float floor)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float m = __uint_as_float(first_bits + i * stride);
    out[i] = __builtin_amdgcn_logf(m + floor) * 0.693147180559945f;
}

#define CHECK(call)                                                                       \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                           \
            fprintf(stderr, "%s failed: %s\n", #call, hipGetErrorString(e_));             \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

int main(int argc, char **argv)
{
    const uint32_t stride = argc > 1 ? (uint32_t)atoi(argv[1]) : 23u;
    const float floors[] = {1e-2f, 1e-3f, 1e-4f, 1e-5f, 1e-30f, 1.0f};
    const uint32_t chunk = 1u << 22;
    float *dev = nullptr;
    CHECK(hipMalloc(&dev, chunk * sizeof(float)));
    std::vector<float> host(chunk);
    for (float floor : floors) {
        // m = 0 and then every stride-th float from the smallest normal number up to 2 - floor
        float top = 2.0f - floor;
        uint32_t top_bits, lo_bits = 0x00800000u;
        memcpy(&top_bits, &top, 4);
        double worst = 0.0, worst_m = 0.0;
        uint64_t visited = 0;
        for (uint64_t b = lo_bits; b <= top_bits; b += (uint64_t)chunk * stride) {
            const uint64_t left = (top_bits - b) / stride + 1;
            const uint32_t n = (uint32_t)(left < chunk ? left : chunk);
            k_map<<<(n + 255) / 256, 256>>>(dev, (uint32_t)b, stride, n, floor);
            CHECK(hipGetLastError());
            CHECK(hipMemcpy(host.data(), dev, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t bits = (uint32_t)b + i * stride;
                float m;
                memcpy(&m, &bits, 4);
                const double err = fabs((double)host[i] - log((double)m + (double)floor));
                if (err > worst) worst = err, worst_m = m;
            }
            visited += n;
        }
        // m = 0: the table entry of an empty target bin
        k_map<<<1, 256>>>(dev, 0u, 0u, 1u, floor);
        CHECK(hipMemcpy(host.data(), dev, sizeof(float), hipMemcpyDeviceToHost));
        const double err0 = fabs((double)host[0] - log((double)floor));
        if (err0 > worst) worst = err0, worst_m = 0.0;
        printf("floor %g: max |ln_dev(m + floor) - log(m + floor)| = %.4g at m = %.9g over %llu arguments (m = 0: %.4g); ulp(|ln floor|) = %.4g\n",
               (double)floor, worst, worst_m, (unsigned long long)visited + 1, err0,
               (double)(nextafterf(fabsf(logf(floor)), INFINITY) - fabsf(logf(floor))));
    }
    CHECK(hipFree(dev));
    return 0;
}
