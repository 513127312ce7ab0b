// Microbenchmark: the back-to-back issue rate of v_mfma_f64_16x16x4_f64 on one SIMD -- the roof that mmvae_gram
// (csrc/pca.hip) is measured against (tools/pca_time.py runs this program and records its last line).
// CHAINS independent accumulators per wave, operands in registers, no memory traffic in the loop; one, two and four waves a
// SIMD.  Prints, per shape, the time per MFMA per SIMD and the TFLOP/s of the whole chip (2048 flops an instruction).
//   hipcc --offload-arch=gfx950 -O3 -Wno-unused-value -o tools/micro/mfma_f64_bench tools/micro/mfma_f64_bench.hip
#include <hip/hip_runtime.h>
#include <stdio.h>
typedef double f64x4 __attribute__((ext_vector_type(4)));

template <int CHAINS>
__global__ __launch_bounds__(256) void k(double* out, int iters, double seed) {
    const int lane = threadIdx.x & 63;
    f64x4 acc[CHAINS];
    for (int c = 0; c < CHAINS; ++c) acc[c] = f64x4{0.0, 0.0, 0.0, 0.0};
    const double a = seed * (lane + 1), b = seed * (64 - lane);
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int c = 0; c < CHAINS; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[c], 0, 0, 0);
    }
    double s = 0.0;
    for (int c = 0; c < CHAINS; ++c) s += acc[c][0] + acc[c][1] + acc[c][2] + acc[c][3];
    out[(size_t)blockIdx.x * 256 + threadIdx.x] = s;
}

template <int CHAINS>
double run(int cus, int waves_per_simd, int iters, double* out, double* tflops) {
    const int blocks = cus * waves_per_simd;             // 256 threads: one wave on each of a CU's four SIMDs
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL(k<CHAINS>, dim3(blocks), dim3(256), 0, 0, out, iters, 1e-3);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    hipLaunchKernelGGL(k<CHAINS>, dim3(blocks), dim3(256), 0, 0, out, iters, 1e-3);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    const double per_simd = (double)iters * CHAINS * waves_per_simd;
    const double ns = ms * 1e6 / per_simd;
    *tflops = (double)blocks * 4 * iters * CHAINS * 2048.0 / (ms * 1e-3) / 1e12;
    printf("chains %d waves/SIMD %d: %9.1f us  %6.2f ns per MFMA per SIMD  %6.2f TFLOP/s\n", CHAINS, waves_per_simd, ms * 1e3, ns, *tflops);
    return ns;
}

int main() {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, 0) != hipSuccess) { fprintf(stderr, "no device\n"); return 1; }
    const int cus = p.multiProcessorCount;
    double* out; hipMalloc(&out, (size_t)cus * 4 * 256 * sizeof(double));
    double best_ns = 1e30, best_tf = 0.0, tf;
    for (int w : {1, 2, 4}) {
        double ns = run<1>(cus, w, 20000, out, &tf); if (tf > best_tf) { best_tf = tf; best_ns = ns; }
        ns = run<4>(cus, w, 5000, out, &tf); if (tf > best_tf) { best_tf = tf; best_ns = ns; }
    }
    printf("f64_16x16x4 cus %d clock_mhz %d best_ns_per_mfma_per_simd %.3f best_tflops %.3f\n", cus, p.clockRate / 1000, best_ns, best_tf);
    return 0;
}
