// Input-gradient-only backward of the fused base-shape DiT (see train_fused.hpp, backward_dx): the d x instantiations of the fused
// backward layer (dit_backward.hpp with SCLDM_BWD_DXONLY) and the final layer's data gradient.  What a log-likelihood solve or an
// input VJP needs per evaluation: no operand pairs, no weight-gradient GEMMs, no adaLN / bias gradients.  gfx950 only.
#include "train_fused.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "api_common.hpp"
#define SCLDM_BWD_DXONLY 1
#define SCLDM_BWD_NTT 2
#define SCLDM_BWD_NS bwd_dx
#define SCLDM_BWD_OP OpBF16
#include "dit_backward.hpp"
#undef SCLDM_BWD_NS
#undef SCLDM_BWD_OP
#define SCLDM_BWD_NS bwdh_dx
#define SCLDM_BWD_OP OpFP16
#include "dit_backward.hpp"
#undef SCLDM_BWD_NS
#undef SCLDM_BWD_OP
#undef SCLDM_BWD_NTT
#define SCLDM_BWD_NTT 1
#define SCLDM_BWD_NS bwd32_dx
#define SCLDM_BWD_OP OpBF16
#include "dit_backward.hpp"
#undef SCLDM_BWD_NS
#undef SCLDM_BWD_OP
#define SCLDM_BWD_NS bwdh32_dx
#define SCLDM_BWD_OP OpFP16
#include "dit_backward.hpp"
#undef SCLDM_BWD_NS
#undef SCLDM_BWD_OP
#undef SCLDM_BWD_NTT
#undef SCLDM_BWD_DXONLY

namespace scldm {
namespace fused {

namespace {

__device__ __forceinline__ size_t tile_addr_dx(long tok, int f) {   // as tile_addr of train_fused.hip: feature f (multiple of 4) of token tok
  const long tile = tok >> 6;
  const int tt = (int)(tok >> 5) & 1, c32 = (int)tok & 31;
  const int wave = f >> 6, ft = (f >> 5) & 1, q = (f >> 3) & 3, hh = (f >> 2) & 1;
  return ((size_t)((tile * 4 + wave) * 16 + (tt * 2 + ft) * 4 + q) * 64 + c32 + 32 * hh) * 4;
}
__device__ __forceinline__ float wave_sum64_dx(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// final_bwd_kernel (train_fused.hip) reduced to its d x: out = (LN(x) (1 + scale) + shift) fin_w^T + b, given dout.  Same walk
// (workgroup -> samples b, b + grid, ...; wave w tokens 4w .. 4w+3; lane l features 4l .. 4l+3) and the same expressions term by term.
template <int DIN>
__global__ __launch_bounds__(256) void final_bwd_dx_kernel(const float* __restrict__ x_last, const float* __restrict__ mod, int mod_stride, int of,
                                                           const float* __restrict__ dout, const float* __restrict__ fin_w, float eps, int n,
                                                           float* __restrict__ dx) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, f = lane * 4;
  f32x4 wq[DIN];
#pragma unroll
  for (int c = 0; c < DIN; ++c) wq[c] = *reinterpret_cast<const f32x4*>(fin_w + (size_t)c * kD + f);
  for (int b = blockIdx.x; b < n; b += gridDim.x) {
    f32x4 scale = *reinterpret_cast<const f32x4*>(mod + (size_t)b * mod_stride + of + kD + f);
    scale += 1.0f;
    for (int tt = 0; tt < 4; ++tt) {
      const long tok = (long)b * 16 + wave * 4 + tt;
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x_last + tile_addr_dx(tok, f));
      const float mean = wave_sum64_dx((xv[0] + xv[1]) + (xv[2] + xv[3])) * (1.0f / kD);
      f32x4 xh = xv - mean;
      const float rstd = 1.0f / sqrtf(wave_sum64_dx((xh[0] * xh[0] + xh[1] * xh[1]) + (xh[2] * xh[2] + xh[3] * xh[3])) * (1.0f / kD) + eps);
      xh *= rstd;
      const float dlane = lane < DIN ? dout[tok * DIN + lane] : 0.f;
      f32x4 dh = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < DIN; ++c) {
        const float d = __shfl(dlane, c);
        dh += d * wq[c];
      }
      const f32x4 g = dh * scale;
      const float s1 = wave_sum64_dx((g[0] + g[1]) + (g[2] + g[3])) * (1.0f / kD);
      const float s2 = wave_sum64_dx((g[0] * xh[0] + g[1] * xh[1]) + (g[2] * xh[2] + g[3] * xh[3])) * (1.0f / kD);
      *reinterpret_cast<f32x4*>(dx + tile_addr_dx(tok, f)) = rstd * (g - s1 - xh * s2);
    }
  }
}

inline int pad4(int n) { return (n + 3) / 4 * 4; }

template <int DIN>
int final_backward_dx_t(scldm_dit* h, const float* x_last, const float* mod, const float* dout, const float* fin_w, int n, float* dx, hipStream_t st) {
  const int of = h->cfg.n_layer * kModBlock, groups = std::min(n, 256);
  if (n % 4)   // ragged batch: the padding samples of the last 64-token tile must enter the layers with a zero gradient
    HIP_TRY(hipMemsetAsync(dx + (size_t)(n / 4) * 64 * kD, 0, (size_t)64 * kD * sizeof(float), st));
  final_bwd_dx_kernel<DIN><<<groups, 256, 0, st>>>(x_last, mod, h->mod_w, of, dout, fin_w, h->cfg.layernorm_eps, n, dx);
  LAUNCH_CHECK();
  return SCLDM_OK;
}

#define SCLDM_BWD_POLICY(NAME, NS_, ETYPE)                                                                                        \
  struct NAME {                                                                                                                  \
    using Args = NS_::BwdArgs;                                                                                                   \
    using E = ETYPE;                                                                                                             \
    static constexpr int NW = NS_::NW, NT = NS_::NT, LDS_BYTES = NS_::LDS_BYTES, TILES_PER_64 = 2 / NS_::NTT;                    \
    static void launch(int tiles, hipStream_t st, const Args& a) { NS_::dit_backward_kernel<<<tiles, NT, LDS_BYTES, st>>>(a); }  \
    static const void* kernel() { return (const void*)NS_::dit_backward_kernel; }                                                \
  }
SCLDM_BWD_POLICY(DxBF16, bwd_dx, __bf16);
SCLDM_BWD_POLICY(DxFP16, bwdh_dx, _Float16);
SCLDM_BWD_POLICY(DxBF16Small, bwd32_dx, __bf16);   // 32-token tiles (the training backward's size rule)
SCLDM_BWD_POLICY(DxFP16Small, bwdh32_dx, _Float16);
#undef SCLDM_BWD_POLICY

template <typename BW>
int backward_layers_dx_t(scldm_dit* h, const float* mod, int n, const Record& rec, const Scratch& s, hipStream_t st) {
  using E16 = typename BW::E;
  static bool attr_set[64] = {};   // (per instantiation)
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !attr_set[dev]) {
    HIP_TRY(hipFuncSetAttribute(BW::kernel(), hipFuncAttributeMaxDynamicSharedMemorySize, BW::LDS_BYTES));
    if (dev >= 0 && dev < 64) attr_set[dev] = true;
  }
  const scldm_dit_config& c = h->cfg;
  const int tiles = pad4(n) / 4 * BW::TILES_PER_64;
  const size_t TD = (size_t)pad4(n) * 16 * kD;
  const size_t bwd_layer_elems = (size_t)BW::NW * kBwdUnitsLayer * 512;
  for (int l = c.n_layer - 1; l >= 0; --l) {
    typename BW::Args a{};   // (dmod and the nine operand-pair pointers stay NULL: this family never forms their addresses)
    a.x_in = rec.x + (size_t)l * TD;
    a.y1 = reinterpret_cast<const E16*>(rec.y1) + (size_t)l * TD;
    a.y2 = reinterpret_cast<const E16*>(rec.y2) + (size_t)l * TD;
    a.dx = s.dx;
    a.mod = mod;
    a.mod_stride = h->mod_w;
    a.mod_off = l * kModBlock;
    a.w_stream = reinterpret_cast<const E16*>(h->bwd_stream) + (size_t)l * bwd_layer_elems;
    a.b_qkv = h->b_qkv + (size_t)l * 768;
    a.n = n;
    a.eps = c.layernorm_eps;
    a.attn_scale = 1.0f / sqrtf(32.0f);
    a.attn_scale_log2e = 1.4426950408889634f / sqrtf(32.0f);
    BW::launch(tiles, st, a);
    LAUNCH_CHECK();
  }
  return SCLDM_OK;
}

}  // namespace

int final_backward_dx(scldm_dit* h, const float* x_last, const float* mod, const float* dout, const float* fin_w, int n, float* dx, hipStream_t st) {
  switch (h->cfg.n_embed_input) {
    case 16: return final_backward_dx_t<16>(h, x_last, mod, dout, fin_w, n, dx, st);
    case 32: return final_backward_dx_t<32>(h, x_last, mod, dout, fin_w, n, dx, st);
    case 8: return final_backward_dx_t<8>(h, x_last, mod, dout, fin_w, n, dx, st);
    default: return fail(SCLDM_ERR_SHAPE, "fused edge kernels are instantiated for n_embed_input 8 / 16 / 32");
  }
}

int backward_layers_dx(scldm_dit* h, const float* mod, int n, const Record& rec, const Scratch& s, hipStream_t st, int precision) {
  // the size rule of backward_layers (train_fused.hip): 32-token tiles while 2 * tiles64 <= kOverlapTiles, SCLDM_TRAIN_SMALL_NTT=0: off
  static const bool small_ok = [] { const char* e = getenv("SCLDM_TRAIN_SMALL_NTT"); return !(e && e[0] == '0'); }();
  if (small_ok && pad4(n) / 4 * 2 <= kOverlapTiles)
    return precision == SCLDM_PREC_FP16 ? backward_layers_dx_t<DxFP16Small>(h, mod, n, rec, s, st) : backward_layers_dx_t<DxBF16Small>(h, mod, n, rec, s, st);
  return precision == SCLDM_PREC_FP16 ? backward_layers_dx_t<DxFP16>(h, mod, n, rec, s, st) : backward_layers_dx_t<DxBF16>(h, mod, n, rec, s, st);
}

}  // namespace fused
}  // namespace scldm
