// scldm_fm_prepare / scldm_fm_loss_grad (train_step.hip) under any transport of transport_path.hpp: the GVP path, noise / score
// prediction, the loss weights.  A translation unit of its own: the kernels of train_step.hip compile to the instructions they had
// before these existed (profiles/transport_paths_isa_identity.txt).
#include <hip/hip_runtime.h>

#include "api_common.hpp"
#include "common.hpp"
#include "fm_step_common.hpp"
#include "transport_path.hpp"

#pragma clang fp contract(off)

namespace scldm {
namespace fmstep {

// ---------------------------------------------------------------------------------------------------------------
// The same two kernels under any transport (transport_path.hpp).  fm_prepare_transport_kernel makes fm_prepare_kernel's Philox calls
// with its counters (the same seed and step give the same uniform u, normals and label decisions), maps u to
// t = u (t1 - t0) + t0 (product and sum rounded separately: `th.rand(...) * (t1 - t0) + t0`, transport.py:106), and plans with the
// row's coefficients: every thread of a row evaluates them from the same t (one double sincos / tan, no exchange).
// ---------------------------------------------------------------------------------------------------------------
struct PrepTransportArgs {
  PrepArgs p;                       // p.ut receives the loss target (ut | x0 | -x0)
  int path, model, weight;
  float t0, span;                   // t = u * span + t0
  float* rowc;                      // (n, 2): {c, w}
};
__global__ __launch_bounds__(256) void fm_prepare_transport_kernel(const PrepTransportArgs ta) {
  const PrepArgs& a = ta.p;
  const unsigned long long seed = a.rng[0], ctr = a.rng[1];
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), s0 = (uint32_t)ctr, s1 = (uint32_t)(ctr >> 32);
  const long q = blockIdx.x * 256l + threadIdx.x, i = q * 4, total = (long)a.n * a.e;
  if (i >= total) return;
  const int row = (int)(i / a.e);
  const U4 r = philox4((uint32_t)row, s0, s1, TAG_ROW, k0, k1);
  const float tv = u01_closed0(r.x) * ta.span + ta.t0;      // (contraction is off in this file: two roundings)
  const U4 g = philox4((uint32_t)q, s0 ^ (uint32_t)(q >> 32), s1, TAG_X0, k0, k1);
  const float r0 = sqrtf(-2.0f * logf(u01(g.x))), r1 = sqrtf(-2.0f * logf(u01(g.z)));
  float s_a, c_a, s_b, c_b;
  sincosf(6.283185307179586f * u01(g.y), &s_a, &c_a);
  sincosf(6.283185307179586f * u01(g.w), &s_b, &c_b);
  const float z[4] = {r0 * c_a, r0 * s_a, r1 * c_b, r1 * s_b};
  const scldm::tpath::RowCoef k = scldm::tpath::row_coef(ta.path, ta.model, ta.weight, tv);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (i + j >= total) break;
    const float x1v = a.x1[i + j];
    a.xt[i + j] = scldm::tpath::plan_xt(k, x1v, z[j]);
    a.ut[i + j] = scldm::tpath::plan_tgt(k, ta.model, x1v, z[j]);
    if (a.x0) a.x0[i + j] = z[j];
  }
  if (i % a.e == 0) {
    a.t[row] = tv;
    ta.rowc[2 * row] = k.c;
    ta.rowc[2 * row + 1] = k.w;
    const bool dropped = a.drop && u01_closed0(r.y) < a.p_drop;
    int chosen = -1;
    if (a.strategy == 0) {
      int avail = 0;
      for (int c = 0; c < a.n_classes; ++c) avail += a.labels_in[c] != nullptr;
      const U4 s = philox4(0u, s0, s1, TAG_STEP, k0, k1);
      int pick = avail > 1 ? (int)(s.x % (uint32_t)avail) : 0;
      for (int c = 0; c < a.n_classes; ++c)
        if (a.labels_in[c] && pick-- == 0) chosen = c;
    }
    for (int c = 0; c < a.n_classes; ++c) {
      const bool live = a.labels_in[c] && (a.strategy == 1 || c == chosen) && !dropped;
      a.labels_out[(size_t)c * a.n + row] = live ? a.labels_in[c][row] : (int64_t)a.null_token[c];
    }
  }
}

// fm_loss_grad_kernel with the row's {c, w}: loss_rows[b] = w mean_e (c m - tgt)^2 in fm_wloss_kernel's order and roundings,
// dm = (1/n) w (2/e) c (c m - tgt) as fm_wloss_bwd_kernel forms it for gloss[b] = 1/n; the same ticketed fixed-order mean and counter advance
__global__ __launch_bounds__(256) void fm_wloss_grad_kernel(const float* __restrict__ m, const float* __restrict__ tgt, const float* __restrict__ rowc,
                                                            float* __restrict__ loss_rows, float* __restrict__ loss_mean, float* __restrict__ dm, int n,
                                                            int e, unsigned int* __restrict__ ticket, unsigned long long* __restrict__ rng) {
  __shared__ float red[4];
  __shared__ bool last;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float gl = 1.0f / (float)n, k = 2.0f / (float)e;
  for (int r = wave; r < kLossRows; r += 4) {
    const long b = (long)blockIdx.x * kLossRows + r;
    if (b >= n) break;
    const float c = rowc[2 * b], w = rowc[2 * b + 1];
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int base = 0; base < e; base += 256) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = base + 64 * q + lane;
        if (i < e) {
          const float d = scldm::tpath::wl_diff(c, m[b * e + i], tgt[b * e + i]);
          s[q] = fmaf(d, d, s[q]);
          dm[b * e + i] = scldm::tpath::wl_grad(gl, w, k, c, d);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s[q] += __shfl_xor(s[q], o);
    if (lane == 0) loss_rows[b] = scldm::tpath::wl_row(w, (s[0] + s[1]) + (s[2] + s[3]), e);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    last = atomicAdd(ticket, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) acc += __builtin_nontemporal_load(loss_rows + i);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    *loss_mean = ((red[0] + red[1]) + (red[2] + red[3])) / (float)n;
    *ticket = 0;
    if (rng) rng[1] += 1ull;
  }
}

}  // namespace fmstep
}  // namespace scldm

using namespace scldm::fmstep;

extern "C" int scldm_fm_prepare_transport(const scldm_transport* tr, const float* x1, const int64_t* const* labels_in, const int* null_tokens,
                                          int n_classes, int strategy, int drop, float p_drop, const unsigned long long* rng_state, int n, int e,
                                          float* t, float* x0, float* xt, float* tgt, float* rowc, int64_t* labels_out, void* stream_) {
  if (!scldm::tpath::transport_valid(tr))
    return fail(SCLDM_ERR_SHAPE, "scldm_fm_prepare_transport: bad transport (Linear | GVP, velocity | noise | score, 0 <= eps < 0.5)");
  if (!x1 || !labels_in || !null_tokens || !rng_state || !t || !xt || !tgt || !rowc || !labels_out || n < 1 || e < 1)
    return fail(SCLDM_ERR_SHAPE, "scldm_fm_prepare_transport: bad argument");
  if (n_classes < 1 || n_classes > 8) return fail(SCLDM_ERR_SHAPE, "scldm_fm_prepare_transport: 1..8 condition classes (got %d)", n_classes);
  if (strategy != 0 && strategy != 1) return fail(SCLDM_ERR_SHAPE, "scldm_fm_prepare_transport: strategy 0 (mutually_exclusive) or 1 (joint)");
  if (e % 4) return fail(SCLDM_ERR_SHAPE, "scldm_fm_prepare_transport: the row length must be a multiple of 4 (got %d)", e);
  PrepTransportArgs ta{};
  PrepArgs& a = ta.p;
  a.x1 = x1; a.n_classes = n_classes; a.strategy = strategy; a.drop = drop; a.p_drop = p_drop; a.rng = rng_state;
  a.t = t; a.x0 = x0; a.xt = xt; a.ut = tgt; a.labels_out = labels_out; a.n = n; a.e = e;
  int present = 0;
  for (int c = 0; c < n_classes; ++c) { a.labels_in[c] = labels_in[c]; a.null_token[c] = null_tokens[c]; present += labels_in[c] != nullptr; }
  if (!present) return fail(SCLDM_ERR_SHAPE, "scldm_fm_prepare_transport: condition holds none of the model's classes");
  if (strategy == 1 && present != n_classes) return fail(SCLDM_ERR_SHAPE, "scldm_fm_prepare_transport: the joint strategy needs every class (nnets.py:449)");
  double t0, t1;
  scldm::tpath::transport_interval(tr, false, &t0, &t1);
  ta.path = tr->path; ta.model = tr->model; ta.weight = tr->weight; ta.t0 = (float)t0; ta.span = (float)(t1 - t0); ta.rowc = rowc;
  const long quads = ((long)n * e + 3) / 4;
  hipLaunchKernelGGL(fm_prepare_transport_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, ta);
  LAUNCH_CHECK();
  return SCLDM_OK;
}

extern "C" int scldm_fm_wloss_grad(const float* m, const float* tgt, const float* rowc, int n, int e, float* loss_rows, float* loss_mean, float* dm,
                                   unsigned int* ticket, unsigned long long* rng_state, void* stream_) {
  if (!m || !tgt || !rowc || !loss_rows || !loss_mean || !dm || !ticket || n < 1 || e < 1) return fail(SCLDM_ERR_SHAPE, "scldm_fm_wloss_grad: bad argument");
  hipLaunchKernelGGL(fm_wloss_grad_kernel, dim3((n + kLossRows - 1) / kLossRows), dim3(256), 0, (hipStream_t)stream_, m, tgt, rowc, loss_rows, loss_mean,
                     dm, n, e, ticket, rng_state);
  LAUNCH_CHECK();
  return SCLDM_OK;
}
