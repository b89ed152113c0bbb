// What a packed fp32 instruction costs in a plain VALU stream: a loop of independent v_pk_fma_f32 against a loop of twice as
// many v_fma_f32 (the same flops), both in inline asm so that the compiler can change neither, at 1, 2 and 5 waves per SIMD
// over a fixed trip count.  Per wave: the s_memtime ticks around the loop; per launch (one that fills the chip): wall time by
// events.  Prints one JSON line.  Built and run by tools/pk_fma_cost.py.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef float v2f __attribute__((ext_vector_type(2)));

constexpr int TRIPS = 20000;   // loop trips per wave
constexpr int PLAIN_PER = 32;  // v_fma_f32 per trip; the packed loop issues half as many v_pk_fma_f32

#define CHECK(x)                                                                      \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                   \
            return 2;                                                                 \
        }                                                                             \
    } while (0)

// 16 accumulators, each updated twice per trip: a = a * m + c, m just below 1 so that the values stay finite and non-trivial
__global__ void __launch_bounds__(256) plain_kernel(const float *in, float *out, unsigned long long *ticks, int trips) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    float a0 = in[gid & 1023], a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7;
    float a8 = a0 + 8, a9 = a0 + 9, a10 = a0 + 10, a11 = a0 + 11, a12 = a0 + 12, a13 = a0 + 13, a14 = a0 + 14, a15 = a0 + 15;
    const float m = 0.99993896484375f, c = in[(gid + 7) & 1023] * 0.001f;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < trips; ++i) {
        asm volatile("v_fma_f32 %0, %0, %16, %17\n v_fma_f32 %1, %1, %16, %17\n v_fma_f32 %2, %2, %16, %17\n v_fma_f32 %3, %3, %16, %17\n"
                     "v_fma_f32 %4, %4, %16, %17\n v_fma_f32 %5, %5, %16, %17\n v_fma_f32 %6, %6, %16, %17\n v_fma_f32 %7, %7, %16, %17\n"
                     "v_fma_f32 %8, %8, %16, %17\n v_fma_f32 %9, %9, %16, %17\n v_fma_f32 %10, %10, %16, %17\n v_fma_f32 %11, %11, %16, %17\n"
                     "v_fma_f32 %12, %12, %16, %17\n v_fma_f32 %13, %13, %16, %17\n v_fma_f32 %14, %14, %16, %17\n v_fma_f32 %15, %15, %16, %17\n"
                     "v_fma_f32 %0, %0, %16, %17\n v_fma_f32 %1, %1, %16, %17\n v_fma_f32 %2, %2, %16, %17\n v_fma_f32 %3, %3, %16, %17\n"
                     "v_fma_f32 %4, %4, %16, %17\n v_fma_f32 %5, %5, %16, %17\n v_fma_f32 %6, %6, %16, %17\n v_fma_f32 %7, %7, %16, %17\n"
                     "v_fma_f32 %8, %8, %16, %17\n v_fma_f32 %9, %9, %16, %17\n v_fma_f32 %10, %10, %16, %17\n v_fma_f32 %11, %11, %16, %17\n"
                     "v_fma_f32 %12, %12, %16, %17\n v_fma_f32 %13, %13, %16, %17\n v_fma_f32 %14, %14, %16, %17\n v_fma_f32 %15, %15, %16, %17\n"
                     : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7), "+v"(a8), "+v"(a9), "+v"(a10),
                       "+v"(a11), "+v"(a12), "+v"(a13), "+v"(a14), "+v"(a15)
                     : "v"(m), "v"(c));
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    out[gid] = ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)) + ((a8 + a9) + (a10 + a11)) + ((a12 + a13) + (a14 + a15));
    if ((threadIdx.x & 63) == 0)
        ticks[gid >> 6] = t1 - t0;
}

// the same 16 accumulators as 8 register pairs, each pair updated twice per trip
__global__ void __launch_bounds__(256) packed_kernel(const float *in, float *out, unsigned long long *ticks, int trips) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const float b = in[gid & 1023];
    v2f a0 = {b, b + 1}, a1 = {b + 2, b + 3}, a2 = {b + 4, b + 5}, a3 = {b + 6, b + 7};
    v2f a4 = {b + 8, b + 9}, a5 = {b + 10, b + 11}, a6 = {b + 12, b + 13}, a7 = {b + 14, b + 15};
    const float cs = in[(gid + 7) & 1023] * 0.001f;
    const v2f m = {0.99993896484375f, 0.99993896484375f}, c = {cs, cs};
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < trips; ++i) {
        asm volatile("v_pk_fma_f32 %0, %0, %8, %9\n v_pk_fma_f32 %1, %1, %8, %9\n v_pk_fma_f32 %2, %2, %8, %9\n v_pk_fma_f32 %3, %3, %8, %9\n"
                     "v_pk_fma_f32 %4, %4, %8, %9\n v_pk_fma_f32 %5, %5, %8, %9\n v_pk_fma_f32 %6, %6, %8, %9\n v_pk_fma_f32 %7, %7, %8, %9\n"
                     "v_pk_fma_f32 %0, %0, %8, %9\n v_pk_fma_f32 %1, %1, %8, %9\n v_pk_fma_f32 %2, %2, %8, %9\n v_pk_fma_f32 %3, %3, %8, %9\n"
                     "v_pk_fma_f32 %4, %4, %8, %9\n v_pk_fma_f32 %5, %5, %8, %9\n v_pk_fma_f32 %6, %6, %8, %9\n v_pk_fma_f32 %7, %7, %8, %9\n"
                     : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
                     : "v"(m), "v"(c));
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    const v2f s = ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7));
    out[gid] = s.x + s.y;
    if ((threadIdx.x & 63) == 0)
        ticks[gid >> 6] = t1 - t0;
}

int main() {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    const int max_waves = 5, max_threads = cus * 256 * max_waves;
    std::vector<float> h_in(1024);
    srand(12345);
    for (float &v : h_in)
        v = 0.5f + (float)rand() / (float)RAND_MAX;
    float *d_in, *d_out;
    unsigned long long *d_ticks;
    CHECK(hipMalloc((void **)&d_in, 1024 * sizeof(float)));
    CHECK(hipMalloc((void **)&d_out, (size_t)max_threads * sizeof(float)));
    CHECK(hipMalloc((void **)&d_ticks, (size_t)(max_threads / 64) * sizeof(unsigned long long)));
    CHECK(hipMemcpy(d_in, h_in.data(), 1024 * sizeof(float), hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    printf("{\"device\": \"%s\", \"cus\": %d, \"lds_per_cu\": %zu, \"trips\": %d, \"plain_per_trip\": %d, \"packed_per_trip\": %d, \"runs\": [", prop.gcnArchName,
           cus, (size_t)prop.maxSharedMemoryPerMultiProcessor, TRIPS, PLAIN_PER, PLAIN_PER / 2);
    const int waves_per_simd[3] = {1, 2, 5};
    bool first = true;
    for (int w : waves_per_simd) {
        // one 256-thread workgroup puts a wave on each SIMD of a CU; each asks for so much LDS that exactly w of them fit a
        // CU, so the cus * w workgroups of the grid are resident at once, w to a CU: w waves on every SIMD
        const size_t lds = (size_t)prop.maxSharedMemoryPerMultiProcessor / (size_t)(w + 1) + 1024;
        CHECK(hipFuncSetAttribute((const void *)plain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        CHECK(hipFuncSetAttribute((const void *)packed_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        const int blocks = cus * w, n_waves = blocks * 4;
        for (int packed = 0; packed < 2; ++packed) {
            std::vector<double> med_cyc, wall_ms;
            double tmin = 0.0, tmax = 0.0; // over the waves of the last repetition
            for (int rep = 0; rep < 4; ++rep) { // (the first repetition warms the clock up and is dropped)
                CHECK(hipEventRecord(e0, 0));
                if (packed)
                    hipLaunchKernelGGL(packed_kernel, dim3(blocks), dim3(256), lds, 0, d_in, d_out, d_ticks, TRIPS);
                else
                    hipLaunchKernelGGL(plain_kernel, dim3(blocks), dim3(256), lds, 0, d_in, d_out, d_ticks, TRIPS);
                CHECK(hipGetLastError());
                CHECK(hipEventRecord(e1, 0));
                CHECK(hipEventSynchronize(e1));
                float ms = 0.0f;
                CHECK(hipEventElapsedTime(&ms, e0, e1));
                std::vector<unsigned long long> t((size_t)n_waves);
                CHECK(hipMemcpy(t.data(), d_ticks, t.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
                std::sort(t.begin(), t.end());
                tmin = (double)t.front();
                tmax = (double)t.back();
                if (rep > 0) {
                    med_cyc.push_back((double)t[t.size() / 2]);
                    wall_ms.push_back(ms);
                }
            }
            std::sort(med_cyc.begin(), med_cyc.end());
            std::sort(wall_ms.begin(), wall_ms.end());
            const double instr = (double)TRIPS * (packed ? PLAIN_PER / 2 : PLAIN_PER);
            // ticks of one wave per instruction of its own, and per instruction issued on its SIMD (w waves share it)
            printf("%s{\"waves_per_simd\": %d, \"kind\": \"%s\", \"wave_ticks_median\": %.0f, \"ticks_per_instr_wave\": %.3f, "
                   "\"ticks_per_instr_simd\": %.3f, \"wall_ms_median\": %.4f, \"wave_ticks_min\": %.0f, \"wave_ticks_max\": %.0f}",
                   first ? "" : ", ", w, packed ? "v_pk_fma_f32" : "v_fma_f32", med_cyc[1], med_cyc[1] / instr, med_cyc[1] / instr / w,
                   wall_ms[1], tmin, tmax);
            first = false;
        }
    }
    printf("]}\n");
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    (void)hipFree(d_ticks);
    return 0;
}
