// The stochastic face of the reference's Sampler (src/scldm/transport/transport.py:269-322, integrators.py:7-75) for the one transport
// this project has (Linear path, velocity model): Euler-Maruyama / stochastic Heun steps, a diffusion schedule D(t) and a noise-free
// last step.  With v = model(x, t), score = (t v - x) / (1 - t) and the SDE drift f = v + D score = c_v v + c_x x
// (c_v = 1 + D t / (1 - t), c_x = -D / (1 - t)), EVERY state update of the solve is
//       x' = a_x x + a_v r + a_w w          r = the CFG-blended model output, w ~ N(0, I)
// with three scalars the host knows per update (scldm_sample_sde in api.hip forms them), so the update rides in the blend kernel that
// runs after the trunk anyway: cfg_blend_sde_kernel = CFG blend + score + diffusion + normal draw + state update, one launch.
// RNG: Philox4x32-10 (Salmon et al., SC'11), key = the 64-bit seed, counter = (index of a group of 4 consecutive elements of the
// GLOBAL state (64 bit), step index, tag) - a value depends on (seed, step, global row, column) only, never on the launch geometry,
// the batch size or how the cells were sharded.  Box-Muller, both branches: 4 normals per Philox call = one f32x4 per thread.
// RNG-dependent by nature and outside the bit-parity claim: the draws are tested statistically, everything downstream of
// them is compared against the reference on recorded noise.
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "dit_aux.hpp"

namespace scldm {
namespace sde {

// ---- the two expressions shared with kernels of dit_aux.hpp, compiled under that header's contraction mode so that they stay the
// ---- same instructions: the CFG blend of cfg_blend_kernel and the timestep MLP of t_embed_kernel
#pragma clang fp contract(fast)

// one pass of dz[B + i] = v[B + i] + sum_p scale[p] * (v[2B + pB + i] - v[B + i]) (cfg_blend_kernel's statement, four elements at once)
__device__ __forceinline__ f32x4 cfg_blend_pass(f32x4 r, const f32x4 c, const f32x4 u, float scale) {
  r += scale * (c - u);
  return r;
}

// t_embed_kernel over an explicit device list of times: block e embeds tlist[e] into temb_all[e] (t_embed_all_kernel hard-codes
// linspace(0, 1); the SDE grid ends at 1 - last_step_size and Heun's second evaluation sits at fp32(t + dt))
__global__ __launch_bounds__(256) void t_embed_list_kernel(const float* __restrict__ tlist, const float* __restrict__ w0t,
                                                           const float* __restrict__ b0, const float* __restrict__ w2t,
                                                           const float* __restrict__ b2, float* __restrict__ temb_all) {
  __shared__ float te[256];
  __shared__ float h1[256];
  const int n = threadIdx.x, e = blockIdx.x;
  {
    const int k = n & 127;
    const float freq = expf(-9.210340371976184f * (float)k / 128.0f);
    const float arg = tlist[e] * freq;
    te[n] = (n < 128) ? cosf(arg) : sinf(arg);
  }
  __syncthreads();
  // (64 weight loads requested together, additions in k order: as t_embed_kernel)
  float s = b0[n];
  for (int k0 = 0; k0 < 256; k0 += 64) {
    float wv[64];
#pragma unroll
    for (int j = 0; j < 64; ++j) wv[j] = w0t[(k0 + j) * 256 + n];
#pragma unroll
    for (int j = 0; j < 64; ++j) s += wv[j] * te[k0 + j];
  }
  h1[n] = silu_f(s);
  __syncthreads();
  float c = b2[n];
  for (int k0 = 0; k0 < 256; k0 += 64) {
    float wv[64];
#pragma unroll
    for (int j = 0; j < 64; ++j) wv[j] = w2t[(k0 + j) * 256 + n];
#pragma unroll
    for (int j = 0; j < 64; ++j) c += wv[j] * h1[k0 + j];
  }
  temb_all[(size_t)e * 256 + n] = c;
}

#pragma clang fp contract(off)   // from here on every product and sum is rounded on its own (the CPU restatement's arithmetic)

// the evaluation times of a solve, handed over by value in chunks (no host-to-device copy: the call stays capturable)
constexpr int kTChunk = 256;
struct TChunk { float t[kTChunk]; };
__global__ __launch_bounds__(kTChunk) void set_tlist_kernel(float* __restrict__ tlist, const TChunk c, int n) {
  if ((int)threadIdx.x < n) tlist[threadIdx.x] = c.t[threadIdx.x];
}

struct U4 { uint32_t x, y, z, w; };
__device__ __forceinline__ U4 philox4(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return U4{c0, c1, c2, c3};
}
__device__ __forceinline__ float u01(uint32_t w) { return ((w >> 8) + 0.5f) * (1.0f / 16777216.0f); }   // (0, 1], 24 bits

constexpr uint32_t kTagNoise = 0x73646577u;   // "sdew": the counter word that keeps these draws apart from the project's other Philox streams

// Where a thread's four elements sit in the GLOBAL state: the local state is (2, B, e) = both CFG halves of cells
// [cell_offset, cell_offset + B) out of cells_total; e % 4 == 0, so a group of four never straddles a row.
struct NoiseGeom {
  unsigned long long seed;
  long long cell_offset, cells_total;
  uint32_t step;
};
__device__ __forceinline__ unsigned long long global_group(long long half, long long cell, int col, int e, const NoiseGeom& g) {
  return (unsigned long long)(((half * g.cells_total + g.cell_offset + cell) * e + col) >> 2);
}
// four standard normals of group `grp` at step g.step.  Hardware transcendentals (v_log_f32 / v_sqrt_f32 / v_sin_f32 / v_cos_f32,
// ~1 ulp; the trigonometric units take revolutions, so the uniform needs no 2 pi and no range reduction): as nb_sample.hpp
__device__ __forceinline__ f32x4 normals4(unsigned long long grp, const NoiseGeom& g) {
  const U4 r = philox4((uint32_t)grp, (uint32_t)(grp >> 32), g.step, kTagNoise, (uint32_t)g.seed, (uint32_t)(g.seed >> 32));
  const float r0 = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u01(r.x)));   // sqrt(-2 ln u) = sqrt(-2 ln 2 log2 u)
  const float r1 = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u01(r.z)));
  const float ua = u01(r.y), ub = u01(r.w);
  return f32x4{r0 * __builtin_amdgcn_cosf(ua), r0 * __builtin_amdgcn_sinf(ua), r1 * __builtin_amdgcn_cosf(ub), r1 * __builtin_amdgcn_sinf(ub)};
}

// the normals of thread q's four elements of a local (2, B, e) state (the host keeps 2 B e / 4 below 2^31: 32-bit index arithmetic)
__device__ __forceinline__ f32x4 state_normals4(uint32_t q, int B, int e, const NoiseGeom& g) {
  const uint32_t e4 = (uint32_t)e >> 2, row = q / e4, col = (q % e4) * 4;
  return normals4(global_group(row / (uint32_t)B, row % (uint32_t)B, (int)col, e, g), g);
}

// out (n_rows, e): the normals the sampler draws at g.step for rows [cell_offset, cell_offset + n_rows) of CFG half `half`
__global__ __launch_bounds__(256) void sde_noise_kernel(float* __restrict__ out, long long n_rows, int e, int half, const NoiseGeom g) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x, e4 = (uint32_t)e >> 2;   // (the host keeps n_rows * e4 below 2^31)
  if (q >= (uint32_t)n_rows * e4) return;
  const uint32_t row = q / e4, col = (q % e4) * 4;
  reinterpret_cast<f32x4*>(out)[q] = normals4(global_group(half, row, (int)col, e, g), g);
}

enum { kNoiseNone = 0, kNoiseArray = 1, kNoisePhilox = 2 };
struct BlendArgs {
  const float* v;       // trunk output: 2B unconditional rows, then P conditional passes of B rows (direct: 2B rows, the result itself)
  const float* x;       // (2B, e) the state the evaluation was made at
  float* out;           // (2B, e) receives a_x x + a_v r + a_w w; may be x itself (state update) or another buffer (Heun's K1 / K2)
  float* traj;          // optional second copy of the result (the returned list of states)
  const float* noise;   // kNoiseArray: (2B, e) caller-supplied normals of this step
  int B, e, P, direct, noise_mode;
  float scale[kMaxClasses];
  float a_x, a_v, a_w;
  NoiseGeom g;
};
// thread = 4 consecutive elements (one Philox call).  State update: (a_x, a_v, a_w) = the step's scalars; drift mode (Heun's K1 / K2):
// out = c_x x + c_v r, i.e. (a_x, a_v, a_w) = (c_x, c_v, 0) with noise_mode kNoiseNone
__global__ __launch_bounds__(256) void cfg_blend_sde_kernel(const BlendArgs a) {
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t half = (size_t)a.B * a.e, half4 = half >> 2;
  if (q >= 2 * half4) return;
  const size_t i = q * 4;
  f32x4 r = reinterpret_cast<const f32x4*>(a.v)[q];
  if (!a.direct && q >= half4) {
    const float* vc = a.v + 2 * half + (i - half);   // pass 0 of these elements; pass p is p * half further
    const f32x4 u = r;
    for (int p = 0; p < a.P; ++p) r = cfg_blend_pass(r, *reinterpret_cast<const f32x4*>(vc + (size_t)p * half), u, a.scale[p]);
  }
  const f32x4 x = reinterpret_cast<const f32x4*>(a.x)[q];
  f32x4 o = x * a.a_x + r * a.a_v;
  if (a.noise_mode != kNoiseNone) {
    f32x4 w;
    if (a.noise_mode == kNoiseArray) w = reinterpret_cast<const f32x4*>(a.noise)[q];
    else w = state_normals4((uint32_t)q, a.B, a.e, a.g);
    o = o + w * a.a_w;
  }
  reinterpret_cast<f32x4*>(a.out)[q] = o;
  if (a.traj) reinterpret_cast<f32x4*>(a.traj)[q] = o;
}

// Heun's first move: x += a_w w, in place (xhat = x + sqrt(2 D(t) dt) w, integrators.py:40-44)
struct PerturbArgs {
  float* x;
  const float* noise;
  int B, e, noise_mode;
  float a_w;
  NoiseGeom g;
};
__global__ __launch_bounds__(256) void sde_perturb_kernel(const PerturbArgs a) {
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t half4 = ((size_t)a.B * a.e) >> 2;
  if (q >= 2 * half4) return;
  f32x4 w;
  if (a.noise_mode == kNoiseArray) w = reinterpret_cast<const f32x4*>(a.noise)[q];
  else w = state_normals4((uint32_t)q, a.B, a.e, a.g);
  f32x4* xp = reinterpret_cast<f32x4*>(a.x);
  xp[q] = xp[q] + w * a.a_w;
}

}  // namespace sde
}  // namespace scldm
