// Which bf16 MFMA shape does the fused forward's GEMM regime run faster: v_mfma_f32_32x32x16_bf16 or v_mfma_f32_16x16x32_bf16?
// On a power-capped part the clock the chip holds under load can depend on the shape, so cycles per FLOP do not decide;
// this probe times both shapes on the SAME work, in the forward kernel's own regime:
//   * 256-thread workgroups, two per CU: 2 waves per SIMD;
//   * each wave owns a 64 (features) x 64 (tokens) fp32 output block, 64 accumulator registers in both forms
//     (32x32: 2 x 2 tiles of 16 registers; 16x16: 4 x 4 tiles of 4 registers);
//   * B = activations, read per k-step by ds_read_b128 from an LDS image [64 tokens][256 k] with the kernel's +16 B row pad;
//   * A = weights, streamed L2 -> VGPR through a buffer-descriptor register ring 8 fragments (128 B per lane) ahead, 64 FLOP per
//     streamed byte; the stream cycles a weight set of `units` x 16 KB: by default 1.5 MB, about one layer, which stays in each
//     XCD's 4 MB L2 as a layer's stream does in the kernel (a 12 MB set - 768 units - drifts out of L2 over a long launch and
//     makes the loop stream-bound, which is not the kernel's regime);
//   * per-k-step issue order pinned as in gemm_pass (ds_read | MFMAs | VMEM refill);
//   * N(0, 1) operands (zero operands hide the effect: the loops are reported on zeros too, as a cycle check).
// Per 32 k-values both forms issue 4 A-fragment loads and 4 B-fragment reads of 16 B per lane and 256 MFMA cycles: the 32x32 form
// 8 MFMAs of 32 cycles, the 16x16 form 16 of 16.
// A second build with -DPROBE_STAMP brackets each workgroup's loop with s_memtime / s_memrealtime (stamps go to a buffer of their own,
// no output depends on them) and reports the in-kernel clock and cycles per k-step (median over workgroups).
//   build: hipcc --offload-arch=gfx950 -O3 tests/perf/mfma_shape_probe.hip -o tests/perf/mfma_shape_probe
//          hipcc --offload-arch=gfx950 -O3 -DPROBE_STAMP tests/perf/mfma_shape_probe.hip -o tests/perf/mfma_shape_probe_stamp
//   run:   mfma_shape_probe [k-steps of 32 per launch] [rounds] [weight-set units of 16 KB]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x)                                                                              \
  do {                                                                                        \
    hipError_t e_ = (x);                                                                      \
    if (e_ != hipSuccess) {                                                                   \
      fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));       \
      exit(1);                                                                                \
    }                                                                                         \
  } while (0)

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

constexpr int kK = 256;                        // k-values in the LDS image (one 256-wide activation row per token)
constexpr int kLdb = kK + 8;                   // elements per LDS row: +16 B pad, as the kernel's activation image
constexpr int kTokens = 64;
constexpr int kLdsElems = 34 * 1024;           // 68 KB per workgroup (the image + unused room): at most two workgroups per CU fit
constexpr int kFragBytes = 64 * 16;            // one fragment: 16 B per lane
constexpr int kUnitBytes = 4 * 4 * kFragBytes; // one 32-k step of the whole workgroup: 4 waves x 4 fragments = 16 KB
constexpr int kMaxUnits = 768;                 // weight set: up to 12 MB (the network's 12.6 MB); default 96 units = 1.5 MB (one layer's 1.57 MB)
constexpr int kRingUnits = 2;                  // 32-k steps of run-ahead: 8 fragments = 32 VGPRs, as the kernel's 4 16-k steps x 2

// SHAPE 32: per 32-k step two 16-k sub-steps; A fragment (ft, sub) = rows 32 ft + (l & 31), k 16 sub + 8 (l >> 5).
// SHAPE 16: A fragment ft = rows 16 ft + (l & 15), k 8 (l >> 4).  The values are random; only the register roles differ.
template <int SHAPE>
__global__ __launch_bounds__(256, 2) void shape_loop(const bf16x8* __restrict__ w, const bf16x8* __restrict__ x, float* __restrict__ out,
                                                     unsigned long long* __restrict__ stamps, int steps, int units) {
  static_assert(kLdsElems >= kTokens * kLdb, "LDS image");
  __shared__ __attribute__((aligned(16))) __bf16 bsm[kLdsElems];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < kTokens * kK / 8; i += 256) {
    const int t = i / (kK / 8), c = i % (kK / 8);
    *reinterpret_cast<bf16x8*>(&bsm[t * kLdb + c * 8]) = x[i];
  }
  __syncthreads();

  const unsigned long long b = reinterpret_cast<unsigned long long>(w);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
  const __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((unsigned long long)hi << 32) | lo), 0, units * kUnitBytes, 0x00020000);
  const unsigned lane_off = (unsigned)lane * 16u + (unsigned)wv * 4u * kFragBytes;
  unsigned unit = 0;   // wave-uniform: the next unit to fetch
  auto fetch = [&](int f) -> bf16x8 {
    union { u32x4 q; bf16x8 v; } u;
    u.q = __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane_off + f * kFragBytes, unit * kUnitBytes, 0);
    return u.v;
  };
  bf16x8 ring[kRingUnits][4];
#pragma unroll
  for (int s = 0; s < kRingUnits; ++s) {
#pragma unroll
    for (int f = 0; f < 4; ++f) ring[s][f] = fetch(f);
    unit = unit + 1 == (unsigned)units ? 0 : unit + 1;
  }

  constexpr int NACC = SHAPE == 32 ? 4 : 16;
  typedef __attribute__((ext_vector_type(SHAPE == 32 ? 16 : 4))) float acc_t;
  acc_t acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = acc_t(0.f);

  // B fragment reads: SHAPE 32 -> token (l & 31) + 32 tt, k 16 sub + 8 (l >> 5); SHAPE 16 -> token (l & 15) + 16 tt, k 8 (l >> 4)
  const __bf16* bbase = SHAPE == 32 ? bsm + (lane & 31) * kLdb + (lane >> 5) * 8 : bsm + (lane & 15) * kLdb + (lane >> 4) * 8;
  auto bread = [&](int j, int kofs) -> bf16x8 {
    return *reinterpret_cast<const bf16x8*>(bbase + (SHAPE == 32 ? 32 : 16) * j * kLdb + kofs);
  };

  // B fragments double-buffered as in gemm_pass: the reads of the NEXT (sub-)step are issued in front of this one's MFMAs
  constexpr int NB = SHAPE == 32 ? 2 : 4;
  bf16x8 bcur[NB];
#pragma unroll
  for (int tt = 0; tt < NB; ++tt) bcur[tt] = bread(tt, 0);
#ifdef PROBE_STAMP
  const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
#endif
  for (int it = 0; it < steps; it += kRingUnits) {
#pragma unroll
    for (int s = 0; s < kRingUnits; ++s) {
      const int k1 = ((it + s + 1) & (kK / 32 - 1)) * 32;   // next step's k (wraps within the 256-wide image)
      if constexpr (SHAPE == 32) {
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
          bf16x8 bnext[2];
#pragma unroll
          for (int tt = 0; tt < 2; ++tt) bnext[tt] = bread(tt, sub == 0 ? k1 - 16 + (k1 == 0 ? kK : 0) : k1);
#pragma unroll
          for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int ft = 0; ft < 2; ++ft)
              acc[ft * 2 + tt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ring[s][ft * 2 + sub], bcur[tt], acc[ft * 2 + tt], 0, 0, 0);
#pragma unroll
          for (int ft = 0; ft < 2; ++ft) ring[s][ft * 2 + sub] = fetch(ft * 2 + sub);
#pragma unroll
          for (int tt = 0; tt < 2; ++tt) bcur[tt] = bnext[tt];
          __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);   // DS read
          __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);   // MFMA
          __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);   // VMEM read
        }
      } else {
        bf16x8 bnext[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) bnext[tt] = bread(tt, k1);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
          for (int ft = 0; ft < 4; ++ft)
            acc[ft * 4 + tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ring[s][ft], bcur[tt], acc[ft * 4 + tt], 0, 0, 0);
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) ring[s][ft] = fetch(ft);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) bcur[tt] = bnext[tt];
        __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 4, 0);
      }
      unit = unit + 1 == (unsigned)units ? 0 : unit + 1;
    }
  }
#ifdef PROBE_STAMP
  const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  if (threadIdx.x == 0) {
    stamps[2 * blockIdx.x] = t1 - t0;
    stamps[2 * blockIdx.x + 1] = r1 - r0;
  }
#endif
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NACC; ++i)
#pragma unroll
    for (int r = 0; r < (SHAPE == 32 ? 16 : 4); ++r) sum += acc[i][r];
  if (sum == 12345.678f) out[blockIdx.x * 256 + threadIdx.x] = sum;   // keeps the loop alive, never true in practice
}

static float normal01() {
  const float u1 = (rand() + 1.f) / ((float)RAND_MAX + 2.f), u2 = rand() / (float)RAND_MAX;
  return sqrtf(-2.f * logf(u1)) * cosf(6.2831853f * u2);
}

int main(int argc, char** argv) {
  const int steps = argc > 1 ? atoi(argv[1]) : 200000;
  const int rounds = argc > 2 ? atoi(argv[2]) : 3;
  const int units = argc > 3 ? atoi(argv[3]) : 96;
  if (units < 1 || units > kMaxUnits) { fprintf(stderr, "units must be in [1, %d]\n", kMaxUnits); return 1; }
  if (steps <= 0 || steps % kRingUnits) { fprintf(stderr, "steps must be a positive multiple of %d\n", kRingUnits); return 1; }
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  const int blocks = 2 * prop.multiProcessorCount;   // two workgroups of 4 waves per CU: 2 waves per SIMD
  const size_t wbytes = (size_t)units * kUnitBytes, xbytes = (size_t)kTokens * kK * 2;
  bf16x8 *d_w, *d_x;
  float* d_out;
  unsigned long long* d_st;
  CHECK(hipMalloc(&d_w, wbytes));
  CHECK(hipMalloc(&d_x, xbytes));
  CHECK(hipMalloc(&d_out, (size_t)blocks * 256 * sizeof(float)));
  CHECK(hipMalloc(&d_st, (size_t)blocks * 2 * sizeof(unsigned long long)));
  CHECK(hipMemset(d_st, 0, (size_t)blocks * 2 * sizeof(unsigned long long)));
  std::vector<__bf16> hw(wbytes / 2), hx(xbytes / 2);
#ifdef PROBE_STAMP
  const char* build = "stamp";
#else
  const char* build = "plain";
#endif
  printf("mfma_shape_probe (%s build): %d workgroups x 4 waves, %d k-steps of 32 per launch, 5 launches per measurement, weight set %d units = %.2f MB\n",
         build, blocks, steps, units, units * (double)kUnitBytes / 1048576.0);
  const double flops = 5.0 * blocks * 4.0 * steps * 2.0 * 64 * 64 * 32;
  const char* fills[2] = {"normal(0,1)", "zero"};
  std::vector<double> tf[2][2];
  for (int fill = 0; fill < 2; ++fill) {
    srand(7);
    for (auto& v : hw) v = (__bf16)(fill == 0 ? normal01() : 0.f);
    for (auto& v : hx) v = (__bf16)(fill == 0 ? normal01() : 0.f);
    CHECK(hipMemcpy(d_w, hw.data(), wbytes, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_x, hx.data(), xbytes, hipMemcpyHostToDevice));
    // >= 2 s of back-to-back launches before the first timed one (the clock settles under load)
    for (int k = 0; k < 16; ++k) {
      shape_loop<32><<<blocks, 256>>>(d_w, d_x, d_out, d_st, steps, units);
      shape_loop<16><<<blocks, 256>>>(d_w, d_x, d_out, d_st, steps, units);
    }
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    for (int rd = 0; rd < (fill == 0 ? rounds : 1); ++rd)
      for (int sh = 0; sh < 2; ++sh) {   // interleaved: 32x32, 16x16, 32x32, ...
        hipEvent_t e0, e1;
        CHECK(hipEventCreate(&e0));
        CHECK(hipEventCreate(&e1));
        CHECK(hipEventRecord(e0));
        for (int k = 0; k < 5; ++k) {
          if (sh == 0) shape_loop<32><<<blocks, 256>>>(d_w, d_x, d_out, d_st, steps, units);
          else shape_loop<16><<<blocks, 256>>>(d_w, d_x, d_out, d_st, steps, units);
        }
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipGetLastError());
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        const double t = flops / ms / 1e9;
        tf[fill][sh].push_back(t);
        printf("fill %-12s round %d  %s: %9.1f ms  %8.1f TFLOP/s  (%.3f of 2.5 PF)", fills[fill], rd, sh == 0 ? "32x32x16" : "16x16x32", ms, t, t / 2500.0);
#ifdef PROBE_STAMP
        std::vector<unsigned long long> st((size_t)blocks * 2);
        CHECK(hipMemcpy(st.data(), d_st, st.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        std::vector<double> clk, cyc;
        for (int i = 0; i < blocks; ++i)
          if (st[2 * i + 1] > 0) {
            clk.push_back((double)st[2 * i] / (double)st[2 * i + 1] * 0.1);   // s_memrealtime ticks at 100 MHz -> GHz
            cyc.push_back((double)st[2 * i] / steps);
          }
        std::sort(clk.begin(), clk.end());
        std::sort(cyc.begin(), cyc.end());
        if (!clk.empty())
          printf("  in-kernel clock %.3f GHz (median of %zu WGs, last launch)  %.1f cycles per 32-k step (2 waves per SIMD)", clk[clk.size() / 2], clk.size(),
                 cyc[cyc.size() / 2]);
#endif
        printf("\n");
        fflush(stdout);
        CHECK(hipEventDestroy(e0));
        CHECK(hipEventDestroy(e1));
      }
  }
  for (int fill = 0; fill < 2; ++fill) {
    auto med = [](std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
    printf("fill %-12s median TFLOP/s: 32x32x16 %.1f  16x16x32 %.1f  ratio 16x16/32x32 = %.3f\n", fills[fill], med(tf[fill][0]), med(tf[fill][1]),
           med(tf[fill][1]) / med(tf[fill][0]));
  }
  CHECK(hipFree(d_w));
  CHECK(hipFree(d_x));
  CHECK(hipFree(d_out));
  CHECK(hipFree(d_st));
  return 0;
}
