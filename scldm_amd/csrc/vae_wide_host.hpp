// Host side of the shape-generic TransformerVAE route shared by its two translation units (vae_wide_api.hip: inference,
// vae_wide_train_api.hip: the training backward): the handle and the launch wrappers of the kernels in vae_wide.hpp.  The wrappers are
// defined in vae_wide_api.hip, the one unit that holds those kernels.
#pragma once
#include <vector>

#include "api_common.hpp"

struct scldm_vaew {
  scldm_vae_config cfg;
  size_t cap_bytes;                     // workspace cap of a cell chunk (SCLDM_VAEW_WS_MB at creation)
  bool loaded;
  bool unshared_theta;
  scldm_vae_weights w;                  // the parameters, read where they live
  std::vector<scldm_vae_block> enc_blocks, dec_blocks;
};

namespace scldm {
namespace vaew_host {
struct Ctx {
  const scldm_vaew* h;
  int prec;
  hipStream_t st;
};
constexpr int kWideMaxEmbed = 1024;      // vaew::kMaxEmbed
int wide_attn_keys_per_split(int hd);    // vaew::attn_keys_per_split
void store(const Ctx& c, const float* X, const float* W, float* out, long long M, int N, int K);
void resid(const Ctx& c, const float* X, const float* W, float* out, long long M, int N, int K, const float* R, int rmod = 0,
           const float* R2 = nullptr, int r2mod = 1, const int64_t* ridx = nullptr, int ridx_max = 0);
void swiglu(const Ctx& c, const float* X, const float* w1, const float* w2, float* out, long long M, int H, int K);
void ln(const Ctx& c, const float* src, float* out, long long rows, int n, const float* w, const float* b, const int64_t* gidx = nullptr,
        const float* counts = nullptr);
void attn(const Ctx& c, const float* Q, size_t q_bs, int q_ld, const float* K, const float* V, size_t kv_bs, int kv_ld, float* O, int cells,
          int M, int S, int heads, float* part = nullptr);
}  // namespace vaew_host
}  // namespace scldm
