// Kernels of the record-free inference path of shapes outside the fused family (scldm_dit_infer_*; host side: infer_wide_api.inc, included
// by train_api.hip) and their launchers.  The GEMM, attention and SwiGLU kernels of the training path are launched as they are; what
// inference adds is the modulation read through a row index (several sample-forwards share one conditioning row) without the LayerNorm
// statistics the backward would read.  A translation unit of its own: the training path's code object is the one it was.  gfx950 only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "api_common.hpp"
#include "common.hpp"
#include "infer_wide.hpp"

namespace scldm {
namespace infer {

constexpr int kS = 16;     // tokens per sample

// (put4 / load4f of train.hpp: arrays that only feed GEMMs are bf16 on the bf16-array route)
template <typename TO>
__device__ __forceinline__ void put4(TO* __restrict__ p, const f32x4& v) {
  if constexpr (sizeof(TO) == 4) {
    *reinterpret_cast<f32x4*>(p) = v;
  } else {
    bf16x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (__bf16)v[e];
    *reinterpret_cast<bf16x4*>(p) = o;
  }
}
template <typename T>
__device__ __forceinline__ f32x4 load4f(const T* p) {
  if constexpr (sizeof(T) == 4) {
    return *reinterpret_cast<const f32x4*>(p);
  } else {
    const bf16x4 v = *reinterpret_cast<const bf16x4*>(p);
    return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
  }
}

// ln_mod_fwd_kernel (train.hpp) with the modulation row of sample b at mod + row_index[b] * mod_stride (row_index == nullptr: row b)
// and no `stats` store.  The arithmetic is ln_mod_fwd_kernel's, expression for expression: with the identity index the results
// have its bits.
template <int NQ, typename TO = float, typename TY = float>
__global__ __launch_bounds__(256) void ln_mod_rows_kernel(const float* __restrict__ x, const float* __restrict__ mod, long mod_stride,
                                                          const int32_t* __restrict__ row_index, int sc_off, int sh_off, float eps,
                                                          long tokens, TO* __restrict__ h, const TY* __restrict__ y = nullptr,
                                                          int g_off = 0, float* __restrict__ x_out = nullptr) {
  constexpr int D = NQ * 256, nq = NQ, kMaxDQ = NQ;
  const int lane = threadIdx.x & 63;
  const long t = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (t >= tokens) return;
  const float* m = mod + (row_index ? (long)row_index[t / kS] : t / kS) * mod_stride;
  f32x4 v[kMaxDQ];
  float sum = 0.f;
#pragma unroll
  for (int q = 0; q < kMaxDQ; ++q)
    if (q < nq) {
      v[q] = *reinterpret_cast<const f32x4*>(x + t * D + q * 256 + lane * 4);
      if (y) {
        f32x4 yv;
        if constexpr (sizeof(TY) == 4) {
          yv = *reinterpret_cast<const f32x4*>(y + t * D + q * 256 + lane * 4);
        } else {
          const bf16x4 yb = *reinterpret_cast<const bf16x4*>(y + t * D + q * 256 + lane * 4);
          yv = f32x4{(float)yb[0], (float)yb[1], (float)yb[2], (float)yb[3]};
        }
        const f32x4 gv = *reinterpret_cast<const f32x4*>(m + g_off + q * 256 + lane * 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[q][i] += gv[i] * yv[i];
        *reinterpret_cast<f32x4*>(x_out + t * D + q * 256 + lane * 4) = v[q];
      }
      sum += (v[q][0] + v[q][1]) + (v[q][2] + v[q][3]);
    }
  const float mean = wave_sum(sum) / (float)D;
  float sq = 0.f;
#pragma unroll
  for (int q = 0; q < kMaxDQ; ++q)
    if (q < nq) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[q][i] -= mean;
        sq += v[q][i] * v[q][i];
      }
    }
  const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)D + eps);
#pragma unroll
  for (int q = 0; q < kMaxDQ; ++q)
    if (q < nq) {
      const f32x4 sc = *reinterpret_cast<const f32x4*>(m + sc_off + q * 256 + lane * 4);
      const f32x4 sh = *reinterpret_cast<const f32x4*>(m + sh_off + q * 256 + lane * 4);
      f32x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = v[q][i] * rstd * (1.0f + sc[i]) + sh[i];
      put4(h + t * D + q * 256 + lane * 4, o);
    }
}

// gate_res_kernel (train.hpp) with the gate row read through row_index: x_out = x + gate[row_index[b]] * y
template <typename TY = float>
__global__ void gate_res_rows_kernel(const float* __restrict__ x, const TY* __restrict__ y, const float* __restrict__ mod,
                                     long mod_stride, const int32_t* __restrict__ row_index, int g_off, long tokens, int D,
                                     float* __restrict__ out) {
  const int dq = D / 4;
  const long total = tokens * dq;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long t = i / dq;
    const int f = (int)(i % dq) * 4;
    const long row = row_index ? (long)row_index[t / kS] : t / kS;
    const f32x4 g = *reinterpret_cast<const f32x4*>(mod + row * mod_stride + g_off + f);
    const f32x4 a = *reinterpret_cast<const f32x4*>(x + t * D + f), b = load4f(y + t * D + f);
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = a[k] + g[k] * b[k];
    *reinterpret_cast<f32x4*>(out + t * D + f) = o;
  }
}

// cond_sum_kernel (train.hpp) with a row stride for the timestep embedding: temb_stride 0 shares ONE embedding (a scalar t) among
// all n rows.  Same sum in the same order: c[i] = temb + table_0[..] + table_1[..] + ...   grid (n, D / 256)
__global__ void cond_sum_rows_kernel(const float* __restrict__ temb, long temb_stride, InferEmbed e, int n, int D, float* __restrict__ c) {
  const int i = blockIdx.x, f = blockIdx.y * 256 + threadIdx.x;
  if (i >= n) return;
  float v = temb[(long)i * temb_stride + f];
  for (int k = 0; k < e.n_classes; ++k) {
    long row = e.labels[k] ? (long)e.labels[k][i] : (long)e.vocab[k];
    row = row < 0 ? 0 : (row > e.vocab[k] ? e.vocab[k] : row);
    v += e.table[k][row * D + f];
  }
  c[(long)i * D + f] = v;
}

// The conditional passes of a CFG evaluation re-read the last `rep` samples: x0 of sample-forward s >= n_direct is the projected
// input of sample n_direct - rep + (s - n_direct) % rep (the input projection runs over the n_direct distinct samples only).
// row = floats per sample (16 tokens x D), a multiple of 4.
__global__ void rep_rows_kernel(float* __restrict__ x0, int n_direct, int rep, int n_fwd, long row) {
  const long rq = row / 4, total = (long)(n_fwd - n_direct) * rq;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long s = i / rq, f = (i - s * rq) * 4;
    const long src = n_direct - rep + s % rep;
    *reinterpret_cast<f32x4*>(x0 + (n_direct + s) * row + f) = *reinterpret_cast<const f32x4*>(x0 + src * row + f);
  }
}

// The times of evaluations [e0, e0 + m) of a fixed-grid solve over torch.linspace(0, 1, steps) (fp32, filled from both ends):
// evaluation e of an Euler solve is at grid point e, of a Heun solve at grid point e / 2 + (e & 1).  The products are rounded before
// the subtraction, as on the host.
__global__ void grid_times_kernel(float* __restrict__ t, int steps, int heun, int e0, int m) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const int e = e0 + i, idx = heun ? e / 2 + (e & 1) : e;
  const float step = __fdiv_rn(1.0f, (float)(steps - 1));
  t[i] = idx < steps / 2 ? __fmul_rn(step, (float)idx) : __fsub_rn(1.0f, __fmul_rn(step, (float)(steps - idx - 1)));
}

}  // namespace infer
}  // namespace scldm

using namespace scldm;
using namespace scldm::infer;

namespace {
inline unsigned ew_grid(long count) { return (unsigned)std::max<long>(1, std::min<long>(cdiv(count, 256), 4096)); }
}  // namespace

#define SCLDM_NQ_SWITCH(nq, CALL)  \
  switch (nq) {                    \
    case 1: { CALL(1); break; }    \
    case 2: { CALL(2); break; }    \
    case 3: { CALL(3); break; }    \
    case 4: { CALL(4); break; }    \
    case 5: { CALL(5); break; }    \
    case 6: { CALL(6); break; }    \
    case 7: { CALL(7); break; }    \
    default: { CALL(8); break; }   \
  }

template <typename TO, typename TY>
static int ln_rows_t(hipStream_t st, int D, const float* x, const TY* y, int g_off, float* x_out, const float* mod, long mw, const int32_t* ridx,
                     int sc_off, int sh_off, float eps, long T, TO* h) {
#define CALL(NQ) hipLaunchKernelGGL((ln_mod_rows_kernel<NQ, TO, TY>), dim3(cdiv(T, 4)), dim3(256), 0, st, x, mod, mw, ridx, sc_off, sh_off, eps, T, h, y, g_off, x_out)
  SCLDM_NQ_SWITCH(D / 256, CALL)
#undef CALL
  LAUNCH_CHECK();
  return SCLDM_OK;
}

int scldm_infer_ln_rows(hipStream_t st, int D, const float* x, const void* y, bool y16, int g_off, float* x_out, const float* mod, long mw,
                        const int32_t* ridx, int sc_off, int sh_off, float eps, long T, void* h, bool h16) {
  if (D % 256 != 0 || D < 256 || D > 2048 || T < 1 || (y && !x_out)) return fail(SCLDM_ERR_SHAPE, "scldm_infer_ln_rows: bad argument");
  const __bf16* yb = reinterpret_cast<const __bf16*>(y);
  const float* yf = reinterpret_cast<const float*>(y);
  if (h16) return (y && y16) ? ln_rows_t(st, D, x, yb, g_off, x_out, mod, mw, ridx, sc_off, sh_off, eps, T, reinterpret_cast<__bf16*>(h))
                             : ln_rows_t(st, D, x, yf, g_off, x_out, mod, mw, ridx, sc_off, sh_off, eps, T, reinterpret_cast<__bf16*>(h));
  return (y && y16) ? ln_rows_t(st, D, x, yb, g_off, x_out, mod, mw, ridx, sc_off, sh_off, eps, T, reinterpret_cast<float*>(h))
                    : ln_rows_t(st, D, x, yf, g_off, x_out, mod, mw, ridx, sc_off, sh_off, eps, T, reinterpret_cast<float*>(h));
}

int scldm_infer_gate_res_rows(hipStream_t st, const float* x, const void* y, bool y16, const float* mod, long mw, const int32_t* ridx, int g_off,
                              long T, int D, float* out) {
  if (y16) hipLaunchKernelGGL(gate_res_rows_kernel<__bf16>, dim3(ew_grid(T * D / 4)), dim3(256), 0, st, x, reinterpret_cast<const __bf16*>(y), mod, mw, ridx, g_off, T, D, out);
  else hipLaunchKernelGGL(gate_res_rows_kernel<float>, dim3(ew_grid(T * D / 4)), dim3(256), 0, st, x, reinterpret_cast<const float*>(y), mod, mw, ridx, g_off, T, D, out);
  LAUNCH_CHECK();
  return SCLDM_OK;
}

int scldm_infer_cond_sum_rows(hipStream_t st, const float* temb, long temb_stride, const InferEmbed& e, int n, int D, float* c) {
  hipLaunchKernelGGL(cond_sum_rows_kernel, dim3(n, D / 256), dim3(256), 0, st, temb, temb_stride, e, n, D, c);
  LAUNCH_CHECK();
  return SCLDM_OK;
}

int scldm_infer_rep_rows(hipStream_t st, float* x0, int n_direct, int rep, int n_fwd, long row) {
  hipLaunchKernelGGL(rep_rows_kernel, dim3(ew_grid((long)(n_fwd - n_direct) * row / 4)), dim3(256), 0, st, x0, n_direct, rep, n_fwd, row);
  LAUNCH_CHECK();
  return SCLDM_OK;
}

int scldm_infer_grid_times(hipStream_t st, float* t, int steps, int heun, int e0, int m) {
  hipLaunchKernelGGL(grid_times_kernel, dim3(cdiv(m, 256)), dim3(256), 0, st, t, steps, heun, e0, m);
  LAUNCH_CHECK();
  return SCLDM_OK;
}
