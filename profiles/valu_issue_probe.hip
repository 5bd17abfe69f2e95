// valu_issue_probe.hip — how many cycles a SIMD of gfx950 takes to issue one VALU instruction of a kind
// (DESIGN.md §6 "what binds k_seg on C3").  Stand-alone:
//
//   hipcc --offload-arch=gfx950 -O3 -o valu_issue_probe profiles/valu_issue_probe.hip && ./valu_issue_probe
//
// One tiny kernel per kind: every wave runs kInstr independent instructions of the kind (eight accumulators in
// rotation, so no instruction waits on the one before it; 512 per loop round, the round's three scalar
// instructions and its taken branch beside them) between two clock64() stamps.  One workgroup per launch: 256 threads put one wave on
// each SIMD of a CU, 1,024 threads four.  The waves meet at a barrier before the first stamp, so the waves of a
// SIMD run their streams together; a SIMD's rate is then (waves on it) x kInstr instructions in the longest of
// its waves' intervals.  HW_ID tells which SIMD a wave ran on, and the table prints how many shared one.
// Reported: cycles per instruction as one wave sees it, and cycles per instruction per SIMD.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kRounds = 16, kPerRound = 512, kInstr = kRounds * kPerRound;

struct Stamp {
    long long t0, t1;
    uint32_t hw_id, pad;
};

enum Kind { FMA32, PKFMA32, FMA64, CNDMASK, MIX_32_64, N_KINDS };
static const char* const kNames[N_KINDS] = {"v_fma_f32", "v_pk_fma_f32", "v_fma_f64", "v_cndmask_b32", "v_fma_f32 + v_fma_f64 1:1"};

// eight lines with eight accumulators, sixty-four times
#define REPT64(body) ".rept 64\n" body ".endr\n"

template <int KIND>
__global__ void __launch_bounds__(1024) k_probe(Stamp* out, float* sink, float seed) {
    const float x = seed + (float)threadIdx.x * 1e-3f, y = 1.0f - 1e-6f * seed;
    long long t0 = 0, t1 = 0;
    float res = 0.0f;
    if constexpr (KIND == FMA32) {
        float a0 = x, a1 = x + 1, a2 = x + 2, a3 = x + 3, a4 = x + 4, a5 = x + 5, a6 = x + 6, a7 = x + 7;
        __syncthreads();
        t0 = clock64();
#pragma unroll 1
        for (int r = 0; r < kRounds; ++r)
            asm volatile(REPT64("v_fma_f32 %0, %0, %8, %9\n v_fma_f32 %1, %1, %8, %9\n v_fma_f32 %2, %2, %8, %9\n v_fma_f32 %3, %3, %8, %9\n"
                                "v_fma_f32 %4, %4, %8, %9\n v_fma_f32 %5, %5, %8, %9\n v_fma_f32 %6, %6, %8, %9\n v_fma_f32 %7, %7, %8, %9\n")
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
                         : "v"(y), "v"(x));
        t1 = clock64();
        res = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;
    } else if constexpr (KIND == PKFMA32) {
        const f32x2 yy = {y, y}, xx = {x, -x};
        f32x2 a0 = {x, x}, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7;
        __syncthreads();
        t0 = clock64();
#pragma unroll 1
        for (int r = 0; r < kRounds; ++r)
            asm volatile(REPT64("v_pk_fma_f32 %0, %0, %8, %9\n v_pk_fma_f32 %1, %1, %8, %9\n v_pk_fma_f32 %2, %2, %8, %9\n v_pk_fma_f32 %3, %3, %8, %9\n"
                                "v_pk_fma_f32 %4, %4, %8, %9\n v_pk_fma_f32 %5, %5, %8, %9\n v_pk_fma_f32 %6, %6, %8, %9\n v_pk_fma_f32 %7, %7, %8, %9\n")
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
                         : "v"(yy), "v"(xx));
        t1 = clock64();
        const f32x2 s = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;
        res = s.x + s.y;
    } else if constexpr (KIND == FMA64) {
        const double yd = y, xd = x;
        double a0 = x, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7;
        __syncthreads();
        t0 = clock64();
#pragma unroll 1
        for (int r = 0; r < kRounds; ++r)
            asm volatile(REPT64("v_fma_f64 %0, %0, %8, %9\n v_fma_f64 %1, %1, %8, %9\n v_fma_f64 %2, %2, %8, %9\n v_fma_f64 %3, %3, %8, %9\n"
                                "v_fma_f64 %4, %4, %8, %9\n v_fma_f64 %5, %5, %8, %9\n v_fma_f64 %6, %6, %8, %9\n v_fma_f64 %7, %7, %8, %9\n")
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
                         : "v"(yd), "v"(xd));
        t1 = clock64();
        res = (float)(a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7);
    } else if constexpr (KIND == CNDMASK) {
        const unsigned long long mask = __builtin_amdgcn_ballot_w64((threadIdx.x & 1) != 0);
        float a0 = x, a1 = x + 1, a2 = x + 2, a3 = x + 3, a4 = x + 4, a5 = x + 5, a6 = x + 6, a7 = x + 7;
        __syncthreads();
        t0 = clock64();
#pragma unroll 1
        for (int r = 0; r < kRounds; ++r)
            asm volatile(REPT64("v_cndmask_b32 %0, %0, %8, %9\n v_cndmask_b32 %1, %1, %8, %9\n v_cndmask_b32 %2, %2, %8, %9\n v_cndmask_b32 %3, %3, %8, %9\n"
                                "v_cndmask_b32 %4, %4, %8, %9\n v_cndmask_b32 %5, %5, %8, %9\n v_cndmask_b32 %6, %6, %8, %9\n v_cndmask_b32 %7, %7, %8, %9\n")
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
                         : "v"(y), "s"(mask));
        t1 = clock64();
        res = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;
    } else {
        const double yd = y, xd = x;
        float a0 = x, a1 = x + 1, a2 = x + 2, a3 = x + 3;
        double a4 = x, a5 = a4 + 1, a6 = a4 + 2, a7 = a4 + 3;
        __syncthreads();
        t0 = clock64();
#pragma unroll 1
        for (int r = 0; r < kRounds; ++r)
            asm volatile(REPT64("v_fma_f32 %0, %0, %8, %9\n v_fma_f64 %4, %4, %10, %11\n v_fma_f32 %1, %1, %8, %9\n v_fma_f64 %5, %5, %10, %11\n"
                                "v_fma_f32 %2, %2, %8, %9\n v_fma_f64 %6, %6, %10, %11\n v_fma_f32 %3, %3, %8, %9\n v_fma_f64 %7, %7, %10, %11\n")
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
                         : "v"(y), "v"(x), "v"(yd), "v"(xd));
        t1 = clock64();
        res = a0 + a1 + a2 + a3 + (float)(a4 + a5 + a6 + a7);
    }
    const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_REG_HW_ID, all 32 bits
    if ((threadIdx.x & 63) == 0) out[threadIdx.x >> 6] = Stamp{t0, t1, hw, 0};
    if (res == 12345.678f) *sink = res;   // keeps the accumulators; never true in practice
}

#define CHECK(e)                                                                                 \
    do {                                                                                         \
        const hipError_t err_ = (e);                                                             \
        if (err_ != hipSuccess) {                                                                \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(err_));    \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)

template <int KIND>
static int run(Stamp* d_out, float* d_sink, int threads, std::vector<Stamp>& st) {
    for (int rep = 0; rep < 3; ++rep) {   // the last launch counts (code and clocks warm)
        hipLaunchKernelGGL(k_probe<KIND>, dim3(1), dim3(threads), 0, 0, d_out, d_sink, 0.5f);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
    }
    st.resize((size_t)threads / 64);
    CHECK(hipMemcpy(st.data(), d_out, st.size() * sizeof(Stamp), hipMemcpyDeviceToHost));
    return 0;
}

int main() {
    Stamp* d_out = nullptr;
    float* d_sink = nullptr;
    CHECK(hipMalloc(&d_out, 16 * sizeof(Stamp)));
    CHECK(hipMalloc(&d_sink, sizeof(float)));
    std::printf("%d independent instructions per wave, one workgroup\n", kInstr);
    // warm the clocks: the first kernels of a process otherwise read up to a quarter slower per instruction
    for (int rep = 0; rep < 3000; ++rep) hipLaunchKernelGGL(k_probe<FMA64>, dim3(1), dim3(1024), 0, 0, d_out, d_sink, 0.5f);
    CHECK(hipDeviceSynchronize());
    std::printf("%-28s %10s %14s %16s %16s\n", "kind", "waves/SIMD", "SIMDs (waves)", "cyc/instr (wave)", "cyc/instr (SIMD)");
    for (int pass = 0; pass < 2; ++pass)   // the whole table twice: the passes should agree
    for (int kind = 0; kind < N_KINDS; ++kind)
        for (int threads : {256, 1024}) {
            std::vector<Stamp> st;
            int rc = 1;
            switch (kind) {
                case FMA32: rc = run<FMA32>(d_out, d_sink, threads, st); break;
                case PKFMA32: rc = run<PKFMA32>(d_out, d_sink, threads, st); break;
                case FMA64: rc = run<FMA64>(d_out, d_sink, threads, st); break;
                case CNDMASK: rc = run<CNDMASK>(d_out, d_sink, threads, st); break;
                default: rc = run<MIX_32_64>(d_out, d_sink, threads, st); break;
            }
            if (rc) return rc;
            // per SIMD (HW_ID bits 5:4): its waves, and the span from their first stamp to their last
            int waves[4] = {0, 0, 0, 0};
            long long lo[4], hi[4];
            double per_wave = 0.0;
            for (const Stamp& s : st) {
                const int simd = (int)((s.hw_id >> 4) & 3);
                lo[simd] = waves[simd] ? std::min(lo[simd], s.t0) : s.t0;
                hi[simd] = waves[simd] ? std::max(hi[simd], s.t1) : s.t1;
                ++waves[simd];
                per_wave += (double)(s.t1 - s.t0) / kInstr;
            }
            per_wave /= (double)st.size();
            double per_simd = 0.0;
            int simds = 0;
            for (int i = 0; i < 4; ++i)
                if (waves[i]) {
                    per_simd += (double)(hi[i] - lo[i]) / ((double)waves[i] * kInstr);
                    ++simds;
                }
            per_simd /= simds;
            std::printf("%-28s %10d   %d (%d,%d,%d,%d) %16.3f %16.3f\n", kNames[kind], threads / 256, simds, waves[0], waves[1], waves[2],
                        waves[3], per_wave, per_simd);
        }
    (void)hipFree(d_out);
    (void)hipFree(d_sink);
    return 0;
}
