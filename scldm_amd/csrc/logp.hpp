// Exact log-likelihood of latents: the probability-flow solve of the reference's Sampler.sample_ode_likelihood
// (src/scldm/transport/transport.py:371-430) over forward_with_cfg (nnets.py:336-378), as device kernels around the recording forward
// and the input-gradient-only backward (scldm_dit_train_forward / scldm_dit_train_backward_dx).
//
// One evaluation at solver time s (model time t = 1 - s) over the doubled CFG state z (2B, e), e = 16 * n_embed_input:
//   rows of the forward  [0, B)            unconditional, x1            seed  eps1
//                        [B, 2B)           unconditional, x2            seed  (1 - sum_p s_p) eps2
//                        [2B + pB, + B)    conditional pass p, x2       seed  s_p eps2
//   v[r]         = u(x1)                                    r <  B      (the CFG blend of cfg_blend_kernel, term by term)
//                = u(x2) + sum_p s_p (c_p(x2) - u(x2))      r >= B
//   dxs[r]       = dx[r]  (r < B),   dx[r] + sum_p dx[2B + pB + r - B]  (r >= B)          = (d v / d x)^T eps
//   logp_grad[r] = sum_j eps[r][j] dxs[r][j]                 (Hutchinson: eps in {-1, +1}, one fresh probe per evaluation)
// and the state moves by -v, delta_logp by +logp_grad (_likelihood_drift, transport.py:391-400).
// RNG: the Philox4x32-10 of sde.hpp, key = the 64-bit seed, counter = (group of 4 consecutive elements of the GLOBAL (2, cells_total, e)
// state, evaluation index, tag): a probe value depends on (seed, evaluation, half, global cell, column) only, so a shard of a solve
// draws what the whole solve would have drawn.  Every reduction is one wave per row in a fixed order (lane-strided partial sums, then
// a butterfly): no atomics, run-to-run identical.  All results leave through plain vector stores.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/scldm_hip.h"
#include "common.hpp"

namespace scldm {
namespace logp {

constexpr int kMaxClasses = SCLDM_MAX_CLASSES;

// one pass of cfg_blend_kernel's statement dz[B + i] = v[B + i] + sum_p scale[p] * (v[2B + pB + i] - v[B + i]) (dit_aux.hpp; four
// elements at once as sde.hpp's cfg_blend_pass), compiled under that kernel's contraction mode so that it stays the same instructions
#pragma clang fp contract(fast)
__device__ __forceinline__ f32x4 cfg_blend_pass(f32x4 r, const f32x4 c, const f32x4 u, float scale) {
  r += scale * (c - u);
  return r;
}

#pragma clang fp contract(off)   // from here on every product and sum is rounded on its own (the CPU restatement's arithmetic)

// Philox4x32-10 (Salmon et al., SC'11) and the global element numbering, as sde.hpp (that header also defines kernels of api.hip's
// translation unit, so it cannot be included twice into the library)
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
// Where a thread's four elements sit in the GLOBAL state: the local state is (2, B, e) = both CFG halves of cells
// [cell_offset, cell_offset + B) out of cells_total; e % 4 == 0, so a group of four never straddles a row.
struct NoiseGeom {
  unsigned long long seed;
  long long cell_offset, cells_total;
  uint32_t step;   // evaluation index
};
__device__ __forceinline__ unsigned long long global_group(long long half, long long cell, int col, int e, const NoiseGeom& g) {
  return (unsigned long long)(((half * g.cells_total + g.cell_offset + cell) * e + col) >> 2);
}

constexpr uint32_t kTagProbe = 0x6c6f6770u;   // "logp": keeps these draws apart from the project's other Philox streams

// four Rademacher values of group `grp` at evaluation g.step: the top bit of each Philox word
__device__ __forceinline__ f32x4 rademacher4(unsigned long long grp, const NoiseGeom& g) {
  const U4 r = philox4((uint32_t)grp, (uint32_t)(grp >> 32), g.step, kTagProbe, (uint32_t)g.seed, (uint32_t)(g.seed >> 32));
  return f32x4{(r.x >> 31) ? 1.f : -1.f, (r.y >> 31) ? 1.f : -1.f, (r.z >> 31) ? 1.f : -1.f, (r.w >> 31) ? 1.f : -1.f};
}

// out (n_rows, e): the probe of evaluation g.step for rows [cell_offset, cell_offset + n_rows) of CFG half `half`
__global__ __launch_bounds__(256) void probe_kernel(float* __restrict__ out, long long n_rows, int e, int half, const NoiseGeom g) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x, e4 = (uint32_t)e >> 2;   // (the host keeps n_rows * e4 below 2^31)
  if (q >= (uint32_t)n_rows * e4) return;
  const uint32_t row = q / e4, col = (q % e4) * 4;
  reinterpret_cast<f32x4*>(out)[q] = rademacher4(global_group(half, row, (int)col, e, g), g);
}

// the per-row labels of the recording forward: null token on the 2B unconditional rows, pass p's classes (mask bit c) on its B rows
struct LabelArgs {
  const int64_t* ulabels[kMaxClasses];   // unique label rows per class (NULL: class unused)
  int64_t* out[kMaxClasses];             // (N) per class
  int null_row[kMaxClasses];
  uint32_t mask[kMaxClasses];
  const int32_t* cell_row;               // cell -> unique label row (NULL: identity)
  int n_classes, B, P;
};
__global__ __launch_bounds__(256) void labels_kernel(const LabelArgs a) {
  const int r = blockIdx.x * 256 + threadIdx.x, N = (2 + a.P) * a.B;
  if (r >= N) return;
  const int p = r < 2 * a.B ? -1 : (r - 2 * a.B) / a.B, i = r < 2 * a.B ? 0 : (r - 2 * a.B) % a.B;
  for (int c = 0; c < a.n_classes; ++c) {
    int64_t l = a.null_row[c];
    if (p >= 0 && ((a.mask[p] >> c) & 1u) && a.ulabels[c]) l = a.ulabels[c][a.cell_row ? a.cell_row[i] : i];
    a.out[c][r] = l;
  }
}

// Probe and seed: thread = 4 consecutive elements of one of the N = (2 + P) B forward rows.  Writes the row's input (its state row),
// its backward seed (coefficient x probe), the probe itself for the 2B state rows, and the row's model time.
struct SeedArgs {
  const float* x;       // (2B, e) the state the evaluation is made at
  const float* probe;   // (2B, e) given probe of this evaluation, or NULL: the generator
  float* xin;           // (N, e)
  float* dout;          // (N, e)
  float* eps;           // (2B, e)
  float* t;             // (N)
  int B, e, P;
  float coef_u;         // 1 - sum_p s_p
  float scale[kMaxClasses];
  float tval;
  NoiseGeom g;
};
__global__ __launch_bounds__(256) void seed_kernel(const SeedArgs a) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x, e4 = (uint32_t)a.e >> 2;   // (the host keeps N * e4 below 2^31)
  const uint32_t N = (uint32_t)(2 + a.P) * (uint32_t)a.B;
  if (q >= N * e4) return;
  const uint32_t r = q / e4, c4 = q % e4, B = (uint32_t)a.B;
  uint32_t half, cell;
  float coef;
  if (r < B) { half = 0; cell = r; coef = 1.f; }
  else if (r < 2 * B) { half = 1; cell = r - B; coef = a.coef_u; }
  else { half = 1; cell = (r - 2 * B) % B; coef = a.scale[(r - 2 * B) / B]; }
  const uint32_t src = half * B + cell;
  f32x4 ep;
  if (a.probe) ep = reinterpret_cast<const f32x4*>(a.probe)[(size_t)src * e4 + c4];
  else ep = rademacher4(global_group(half, cell, (int)(c4 * 4), a.e, a.g), a.g);
  reinterpret_cast<f32x4*>(a.xin)[q] = reinterpret_cast<const f32x4*>(a.x)[(size_t)src * e4 + c4];
  reinterpret_cast<f32x4*>(a.dout)[q] = ep * coef;
  if (r < 2 * B) reinterpret_cast<f32x4*>(a.eps)[q] = ep;
  if (c4 == 0) a.t[r] = a.tval;
}

__device__ __forceinline__ float wave_sum_fixed(float v) {   // butterfly over the 64 lanes: every lane ends with the same bits
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
  return v;
}

enum { kEuler = 0, kHeun1 = 1, kHeun2 = 2 };
// Blend and reduce: one wave per state row r.  mode kEuler: z += hs (-v), dl += hs lg.  kHeun1: k1v = -v, k1l = lg, ztmp = z + hs (-v).
// kHeun2: z += hs (k1v + (-v)), dl += hs (k1l + lg)   (hs = h / 2 there).
struct BlendArgs {
  const float* out;     // (N, e) forward outputs
  const float* dx;      // (N, e) input gradients of the seeded backward
  const float* eps;     // (2B, e)
  float* z;             // (2B, e) the solve's state
  float* ztmp;          // (2B, e) Heun's predictor
  float* k1v;           // (2B, e)
  float* k1l;           // (2B)
  float* dl;            // (2B) delta_logp
  float* traj;          // (2B) this evaluation's logp_grad, or NULL
  int B, e, P, mode;
  float hs;
  float scale[kMaxClasses];
};
__global__ __launch_bounds__(256) void blend_kernel(const BlendArgs a) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= 2 * a.B) return;   // (whole waves leave: the shuffles below see full waves)
  const int e4 = a.e >> 2;
  const size_t half4 = (size_t)a.B * e4, row4 = (size_t)r * e4;
  const f32x4* out = reinterpret_cast<const f32x4*>(a.out);
  const f32x4* dx = reinterpret_cast<const f32x4*>(a.dx);
  float acc = 0.f;
  for (int c4 = lane; c4 < e4; c4 += 64) {
    f32x4 v = out[row4 + c4], d = dx[row4 + c4];
    if (r >= a.B) {
      const f32x4 u = v;
      for (int p = 0; p < a.P; ++p) {
        v = cfg_blend_pass(v, out[row4 + half4 + (size_t)p * half4 + c4], u, a.scale[p]);   // (cfg_blend_kernel's statement)
        d = d + dx[row4 + half4 + (size_t)p * half4 + c4];
      }
    }
    const f32x4 ep = reinterpret_cast<const f32x4*>(a.eps)[row4 + c4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc = acc + ep[i] * d[i];
    const f32x4 nv = -v;
    f32x4* zp = reinterpret_cast<f32x4*>(a.z) + row4 + c4;
    if (a.mode == kEuler) {
      *zp = *zp + nv * a.hs;
    } else if (a.mode == kHeun1) {
      reinterpret_cast<f32x4*>(a.k1v)[row4 + c4] = nv;
      reinterpret_cast<f32x4*>(a.ztmp)[row4 + c4] = *zp + nv * a.hs;
    } else {
      *zp = *zp + (reinterpret_cast<const f32x4*>(a.k1v)[row4 + c4] + nv) * a.hs;
    }
  }
  const float lg = wave_sum_fixed(acc);
  if (lane == 0) {
    if (a.traj) a.traj[r] = lg;
    if (a.mode == kEuler) a.dl[r] = a.dl[r] + lg * a.hs;
    else if (a.mode == kHeun1) a.k1l[r] = lg;
    else a.dl[r] = a.dl[r] + (a.k1l[r] + lg) * a.hs;
  }
}

// End of solve: logp[r] = prior_logp(z[r]) - dl[r], prior_logp(z) = c0 - sum z^2 / 2, c0 = -e / 2 log 2 pi (transport.py:59-67)
__global__ __launch_bounds__(256) void final_kernel(const float* __restrict__ z, const float* __restrict__ dl, int rows, int e, float c0,
                                                    float* __restrict__ logp) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int e4 = e >> 2;
  float acc = 0.f;
  for (int c4 = lane; c4 < e4; c4 += 64) {
    const f32x4 v = reinterpret_cast<const f32x4*>(z)[(size_t)r * e4 + c4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc = acc + v[i] * v[i];
  }
  const float ss = wave_sum_fixed(acc);
  if (lane == 0) logp[r] = (c0 - ss * 0.5f) - dl[r];
}

// The blend under a transport other than the default (transport_path.hpp: Linear | GVP x velocity | noise | score): the probability-flow
// drift is f = a x + b m with m the CFG-blended model output and x the state the evaluation was made at - rows [0, 2B) of the forward's
// input xin, which seed_kernel filled from z (Euler, Heun's first evaluation) or from ztmp (Heun's second).  The state moves by -f and
//   logp_grad = eps . (d f / d x)^T eps = a e + b (eps . (d m / d x)^T eps)          (eps in {-1, +1}: eps . eps = e exactly)
// formed as lg = ae + b * dot: ae = the host's (float)(a * e), dot = the unscaled wave sum of blend_kernel, two roundings.  a, b and ae
// are evaluated in double at the fp32 model time and rounded once on the host.  One wave per row, the fixed butterfly order, plain
// vector stores, as blend_kernel; modes as there.
struct BlendTransportArgs {
  BlendArgs k;          // blend_kernel's arguments
  const float* xin;     // (N, e) the forward's input: rows [0, 2B) = the state of this evaluation
  float a, b, ae;
};
__global__ __launch_bounds__(256) void blend_transport_kernel(const BlendTransportArgs t) {
  const BlendArgs& a = t.k;
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= 2 * a.B) return;   // (whole waves leave: the shuffles below see full waves)
  const int e4 = a.e >> 2;
  const size_t half4 = (size_t)a.B * e4, row4 = (size_t)r * e4;
  const f32x4* out = reinterpret_cast<const f32x4*>(a.out);
  const f32x4* dx = reinterpret_cast<const f32x4*>(a.dx);
  float acc = 0.f;
  for (int c4 = lane; c4 < e4; c4 += 64) {
    f32x4 v = out[row4 + c4], d = dx[row4 + c4];
    if (r >= a.B) {
      const f32x4 u = v;
      for (int p = 0; p < a.P; ++p) {
        v = cfg_blend_pass(v, out[row4 + half4 + (size_t)p * half4 + c4], u, a.scale[p]);   // (cfg_blend_kernel's statement)
        d = d + dx[row4 + half4 + (size_t)p * half4 + c4];
      }
    }
    const f32x4 ep = reinterpret_cast<const f32x4*>(a.eps)[row4 + c4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc = acc + ep[i] * d[i];
    const f32x4 x = reinterpret_cast<const f32x4*>(t.xin)[row4 + c4];
    const f32x4 px = x * t.a, pm = v * t.b;
    const f32x4 nv = -(px + pm);
    f32x4* zp = reinterpret_cast<f32x4*>(a.z) + row4 + c4;
    if (a.mode == kEuler) {
      *zp = *zp + nv * a.hs;
    } else if (a.mode == kHeun1) {
      reinterpret_cast<f32x4*>(a.k1v)[row4 + c4] = nv;
      reinterpret_cast<f32x4*>(a.ztmp)[row4 + c4] = *zp + nv * a.hs;
    } else {
      *zp = *zp + (reinterpret_cast<const f32x4*>(a.k1v)[row4 + c4] + nv) * a.hs;
    }
  }
  const float dot = wave_sum_fixed(acc);
  if (lane == 0) {
    const float bd = t.b * dot;
    const float lg = t.ae + bd;
    if (a.traj) a.traj[r] = lg;
    if (a.mode == kEuler) a.dl[r] = a.dl[r] + lg * a.hs;
    else if (a.mode == kHeun1) a.k1l[r] = lg;
    else a.dl[r] = a.dl[r] + (a.k1l[r] + lg) * a.hs;
  }
}

#pragma clang fp contract(fast)   // back to the compiler's default for whatever the including translation unit defines after this header

}  // namespace logp
}  // namespace scldm
