// libitsd_hip runtime: the C ABI of include/itsd.h.
//
// Builds the UNet op program natively from the reference constructor arguments
// (Diffusion/Model.py:212-262, DiffusionFreeGuidence/ModelCondition.py:164-203),
// repacks the state_dict into MFMA-friendly layouts, owns one activation arena
// sized for max_batch (288 GB of HBM makes a dedicated buffer per op affordable),
// and drives the ancestral sampler loop (Diffusion.py:84-102) as one hipGraph
// replayed T times; the timestep lives in device memory so the graph is
// step-invariant and no host sync happens inside the loop.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "itsd.h"

namespace itsd {
template <typename T> hipError_t launch_conv(const ConvArgs&, const ConvPlan&, hipStream_t);
template <typename T> hipError_t launch_groupnorm(const GNArgs&, int, hipStream_t);
template <typename T> hipError_t launch_attn(const AttnArgs&, int, hipStream_t);
bool attn_flash_ok(int S, int C);
bool attn_cs_ok(int S, int C);
bool attn_block_ok(int S, int C);
hipError_t launch_attn_block(const AttnBlockArgs&, int, hipStream_t);
int g_attn_fuse = 1;  // fused AttnBlock kernel at S = 64 (Arch A's 8x8 level): 0 off, 1 on (itsd_set_option "attn_fuse", read at create)
int g_tap_prune = 1;   // drop conv taps that read only padding for every output pixel ("tap_prune", read at create)
int g_down_merge = 1;  // CFG DownSample c1 (3x3) + c2 (5x5) as one 5x5 conv ("down_merge", read at create)
int g_attn_s1 = 1;    // one-token AttnBlock (the CFG 1x1 level) as GroupNorm + one folded 1x1 conv ("attn_s1", read at create)
template <typename T> hipError_t launch_head(const HeadArgs&, hipStream_t);
template <typename T> hipError_t launch_tail(const TailArgs&, hipStream_t);
hipError_t launch_emb_input(const int*, int, const float*, const float*, int, float*, int, hipStream_t);
hipError_t launch_linear(const float*, int, int, const float*, const float*, int, int, float*, hipStream_t);
hipError_t launch_verify(int, const float*, int, int, int, int, int, double*, const float*, hipStream_t);
hipError_t launch_set_int(int*, int, hipStream_t);
hipError_t launch_add_int(int*, int, hipStream_t);
int calibrate_run(int what, double* value, hipStream_t s);
hipError_t launch_run_begin(int*, int, int*, RunParams*, const RunParams&, hipStream_t);
int g_option_gen = 0;  // bumped by every itsd_set_option: part of the step-graph cache key
bool conv_gn_eligible(int H, int W);  // (shape-only: the op builder's; every per-launch choice is plan_conv's, common.h)
bool p5_eligible(int H, int W);
hipError_t launch_gn_coef(const GNArgs&, int, float*, hipStream_t);
hipError_t launch_head_mfma(const HeadArgs&, hipStream_t);
hipError_t launch_tail_mfma(const TailArgs&, hipStream_t);
bool tail_mfma_ok(int H, int W, int C);
bool tail_block_straddles(int H, int W, int C);
int g_io_mfma = 1;  // bf16 head / tail on MFMA (itsd_set_option "io_mfma", read at create)
int g_small_gn = 1;  // conv_small writes its consumer GroupNorm's output (itsd_set_option "small_gn"): 0 off, 1 on
int g_cfg_skip = 1;  // w == 0 rows of a guidance table run the cond-only step program (itsd_set_option "cfg_skip")
hipError_t launch_noise(float*, const float*, int, long long, float, unsigned long long, unsigned, long long,
                        hipStream_t);
hipError_t launch_branch(float*, const float*, const int*, int, long long, float, float, unsigned long long, unsigned,
                         long long, hipStream_t);
hipError_t launch_probe_noise(float*, const float*, const float*, int, long long, float, float, unsigned long long,
                              unsigned, hipStream_t);
hipError_t launch_es_candidates(float*, const float*, int, long long, float, unsigned long long, unsigned, long long,
                                hipStream_t);
long long es_blocks(long long per_cand);
long long es_workspace_bytes(int n_pairs, long long per_cand);
hipError_t launch_es_step(float*, float*, float*, const float*, int, long long, unsigned long long, unsigned,
                          const EsAdam&, float*, double*, void*, hipStream_t);
template <typename T> hipError_t launch_nhwc_to_nchw(const void*, float*, int, int, int, hipStream_t);
}  // namespace itsd

using namespace itsd;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIPCHK(x)                                                                           \
  do {                                                                                      \
    hipError_t e_ = (x);                                                                    \
    if (e_ != hipSuccess) return fail(ITSD_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

#define CHK(x)                  \
  do {                          \
    int r_ = (x);               \
    if (r_ != ITSD_OK) return r_; \
  } while (0)

// ITSD_ERR_HANDOFF's message from the status word's bits (AttnBlockArgs::err)
std::string handoff_msg(int bits) {
  std::string m = "in-kernel hand-off wait exhausted its poll bound (grid not co-resident?):";
  if (bits & 1) m += " attn_block_split_kernel";
  if (bits & 2) m += " conv3x3_gn_p5_kernel (split-K combine)";
  return m;
}

uint16_t host_f2bf(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// NHWC activation buffer (capacity = max batch), located at ws + off.
struct Act {
  size_t off;
  int H, W, C;
  size_t stats = SIZE_MAX;  // ws offset of the channel-statistics slab (consumed by a GroupNorm), or none
  int spi = 0;              // its slots per image (0: H*W / stat_slot_px(H*W); sub-pixel outputs: stat_spi)
};

enum OpKind { OP_GN, OP_CONV, OP_ATTN, OP_GNCOEF, OP_ATTNBLOCK };
constexpr int kCensusAttnBlock = 7;  // census kind of OP_ATTNBLOCK (runtime.py "attnblock")
constexpr int kCensusConvGN = 4;  // census kind of a fused GroupNorm+SiLU conv (conv3x3_gn_kernel)
constexpr int kCensusConvGNW = 5;   // ... whose shape has 256-pixel tiles of one image's rows (ConvPlan::wide_segs 1)
constexpr int kCensusConvGNW4 = 6;  // ... of four 8x8 images (wide_segs 4)

struct Op {
  OpKind kind;
  int src1 = -1, src2 = -1, dst = -1;
  // GN
  size_t gamma = 0, beta = 0;  // fp32 offsets in the weight arena
  int silu = 0;
  // CONV
  int ksize = 3, stride = 1, pad = 1, upsample = 0, zins = 0;
  int subpix = 0;  // upsample conv as 4 phase-wise 2x2 convs (conv.hip conv_pipe)
  size_t wt = 0, bias = 0;
  size_t wfrag = SIZE_MAX;  // fragment-ordered copy of wt (fused GroupNorm convs: conv3x3_gn_p4 / p5_kernel)
  int Cout = 0, K = 0;
  int temb_col = -1;
  int resid = -1;
  // ATTN
  int S = 0, C = 0;
  int vt = -1, vt_from = 0;  // channel-major V buffer (conv: couts >= vt_from go there; attn: reads it)
  size_t coef = SIZE_MAX;    // GNCOEF: output; CONV: GroupNorm+SiLU coefficients of the input (fused conv)
  size_t bias2 = 0;  // ATTNBLOCK: the proj bias bp; wt / bias: the folded [M | W'] rows (fragment-packed) and [u | b']
  size_t gn_gamma = SIZE_MAX, gn_beta = SIZE_MAX;  // CONV with coef: its input GroupNorm's affine (gn_fold)
  // a ResBlock's block2 conv and its 1x1 shortcut (conv3x3_gn_p5_kernel folds the shortcut in as K slices, ConvArgs
  // sc_*): on block2, the shortcut op, its weights in fragment order and the two biases summed; on the shortcut, block2
  int sc_op = -1, sc_into = -1;
  size_t sc_wfrag = SIZE_MAX, bias_sc = SIZE_MAX;
  // a conv and the GroupNorm op right after it over its output alone (conv_small writes the GroupNorm's output in its
  // epilogue, ConvArgs gn_out): on the conv, the GN op; on the GN op, the conv
  int gn_next = -1, gn_from = -1;
  // introspection (itsd_unet_op_info): the state_dict prefix the op was built from, and ITSD_TAG_* where its weights
  // are not one state_dict tensor
  std::string name;
  int tag = ITSD_TAG_NONE;
};

// Host staging for the weight arena: fp32 params and packed conv weights.
struct Arena {
  std::vector<char> host;
  size_t add(const void* p, size_t bytes) {
    size_t off = (host.size() + 255) & ~(size_t)255;
    host.resize(off + bytes);
    if (p) std::memcpy(host.data() + off, p, bytes);
    return off;
  }
};

// A captured denoising step is keyed by what its launches bake in: the batch, whether labels
// are used, the injected-noise pointer and the kernel-selection options. x and labels are
// staged through handle-owned buffers and the seed, noise offset and clip step live in device
// memory (RunParams), so every round of a search replays one graph.
struct GraphEntry {
  // (n, labels, noise, option generation, schedule form, trace, trace stride, guidance table 0 | 1 | 2, cond-only)
  std::tuple<int, bool, const float*, int, int, const double*, int, int, bool> key;
  hipGraphExec_t exec = nullptr;
};

}  // namespace

struct itsd_unet {
  itsd_unet_desc d{};
  int device = 0;
  bool bf16 = false;
  size_t esz = 4;
  bool cfg = false;
  int H = 32, ch = 128, tdim = 512, sumC = 0;
  int nb_max = 0;  // capacity in images (CFG: 2 * max_batch)
  int last_forward_n = 0;  // batch of the last itsd_unet_forward (itsd_unet_representation reads its tail input)

  char* wdev = nullptr;
  char* ws = nullptr;
  size_t ws_bytes = 0;
  std::vector<Act> acts;
  std::vector<Op> ops;
  int head_out = -1, tail_g = -1, tail_in = -1;
  size_t tail_gn_g = 0, tail_gn_b = 0;

  // fp32 params (arena offsets)
  size_t head_w = 0, head_b = 0, tail_w = 0, tail_b = 0;
  size_t head_wmf = SIZE_MAX, tail_wmf = SIZE_MAX, tail_coef = SIZE_MAX;  // bf16 MFMA head / tail (+ tail GN coefficients)
  size_t freq = 0, ttable = 0, W0t = 0, b0 = 0, W2t = 0, b2 = 0, Wpt = 0, bp = 0;
  size_t ctable = 0, C1t = 0, cb1 = 0, C3t = 0, cb3 = 0, Wct = 0, bc = 0;

  // scratch (separate allocation)
  float* emb_buf = nullptr;   // [rows][ch]
  float* h1_buf = nullptr;    // [rows][tdim]
  float* te_buf = nullptr;    // [rows][tdim]
  float* proj_buf = nullptr;  // [max_batch][sumC]
  int rows_cap = 0;
  float* cemb_table = nullptr;  // [num_labels+1][sumC] (CFG)
  // sampler
  int T_sched = 0;
  float* coeff1 = nullptr;
  float* coeff2 = nullptr;
  float* sqrt_var = nullptr;
  float* temb_table = nullptr;  // [T_sched][sumC]
  // x0-form schedule (itsd_set_schedule_x0): sched_form 1, T_sched = its rows K, temb_table row k = timestep tau[k]'s,
  // xrow = one allocation [5][K] (a0 | b0 | c0 | cx | sg); the three ancestral tables are then null, and the reverse
  // 2M schedule (itsd_set_schedule_x0_2m): sched_form 2, xrow = [6][K] with cp last; x0_hist = the previous row's x0
  // [max_batch][3][H][W] fp32, allocated at the first such call and kept; hist_row / hist_n = the row whose x0 it holds
  // and for how many images (-1 / 0: nothing a continued run may read)
  int sched_form = 0;
  float* xrow = nullptr;
  int clip_x0 = 0;
  float* x0_hist = nullptr;
  int hist_row = -1, hist_n = 0;
  float guide_w = 0.f, guide_w1 = 1.f;
  // the guidance table (itsd_set_guidance): guidance 0 none, 1 rows, 2 rows and per-image multipliers. gw_rows_h /
  // gw_img_h are the host's copies (the cond-only decision and itsd_sampler_predict_x0's scalar read them); gw_rows_d
  // [gw_rows_cap >= T_sched] and gw_img_d [max_batch] are the device's, allocated at the first attach and kept, so a
  // re-install changes values under the captured graphs, never an address
  int guidance = 0;
  std::vector<float> gw_rows_h, gw_img_h;
  float* gw_rows_d = nullptr;
  int gw_rows_cap = 0;
  float* gw_img_d = nullptr;
  int cond_only_steps = 0;  // of the last itsd_sampler_run (itsd_unet_query)
  int* d_t = nullptr;
  int* d_nan = nullptr;
  RunParams* d_run = nullptr;
  float* x_state = nullptr;     // [max_batch][3][H][W]: the sampler's x between the caller's copies
  int32_t* lab_state = nullptr; // [max_batch] labels of the guided sampler
  // itsd_verify_denoise's scratch, allocated at its first call: the noised probe x_t [max_batch][3][H][W] and the tail's
  // per-block partial pairs [max_batch][H W / 64 blocks at most][2]
  float* vd_xt = nullptr;
  float* vd_part = nullptr;
  // the score trace (itsd_sampler_set_trace): the caller's buffer [trace_rows][trace_stride][4] fp64, null while
  // detached, and the tail's per-block partials [max_batch][H W / 64 blocks at most][4], allocated at the first attach
  double* trace = nullptr;
  int trace_rows = 0, trace_stride = 0;
  float* tr_part = nullptr;
  long long graph_captures = 0;  // step graphs captured + instantiated (itsd_unet_query)
  void* zero_page = nullptr;  // 256 KiB of zeros (conv DMA source for padding, conv.hip zero_of_block)
  float* splitk_ws = nullptr;  // split-K partial tiles (shared by all convs: they run in stream order)
  int* tickets = nullptr;      // in-launch split-K counters (conv3x3_gn_p5_kernel), zero between launches
  int* attn_sync = nullptr;    // attn_block_split_kernel's per-image hand-off counter [nb_max] (monotonic)
  static constexpr long long kSplitkCap = 16ll << 20;  // floats (64 MB)

  hipStream_t stream = nullptr;
  hipEvent_t ev_in = nullptr, ev_out = nullptr;
  std::vector<GraphEntry> graphs;

  template <typename P = float>
  P* wp(size_t off) const { return (P*)(wdev + off); }
  void* ap(int id) const { return ws + acts[id].off; }
};

namespace {

struct Builder {
  itsd_unet* u;
  Arena ar;
  std::unordered_map<std::string, std::pair<const float*, int64_t>> w;
  size_t used = 0;
  size_t ws_off = 0;
  std::string err;
  std::vector<std::pair<std::string, size_t>> temb_cols;  // resblock prefix -> column

  const float* get(const std::string& name, int64_t numel) {
    auto it = w.find(name);
    if (it == w.end()) {
      if (err.empty()) err = "missing key in state_dict: " + name;
      return nullptr;
    }
    if (it->second.second != numel) {
      if (err.empty())
        err = "size mismatch for " + name + ": got " + std::to_string(it->second.second) + " elements, expected " +
              std::to_string(numel);
      return nullptr;
    }
    ++used;
    return it->second.first;
  }
  // a second view of an entry already consumed by get/f32 (not counted again)
  const float* peek(const std::string& name, int64_t numel) {
    auto it = w.find(name);
    return (it == w.end() || it->second.second != numel) ? nullptr : it->second.first;
  }
  size_t f32(const std::string& name, int64_t numel) {
    const float* p = get(name, numel);
    return ar.add(p, numel * 4);
  }
  int act(int H, int W, int C) {
    Act a{ws_off, H, W, C};
    size_t bytes = (size_t)u->nb_max * H * W * C * u->esz;
    ws_off = (ws_off + bytes + 255) & ~(size_t)255;
    u->acts.push_back(a);
    return (int)u->acts.size() - 1;
  }
  // Packs conv weight(s) [Cout][Cin][k][k] into [Cout][K] with k = (ky*ks+kx)*Cin + ci.
  // flip_t: source is ConvTranspose2d [Cin][Cout][k][k]; use the flipped kernel.
  size_t pack(const std::vector<const float*>& parts, int Cpart, int Cin, int ks, bool flip_t = false) {
    const int Cout = Cpart * (int)parts.size();
    const int K = ks * ks * Cin;
    std::vector<float> tmp((size_t)Cout * K, 0.f);
    for (size_t pi = 0; pi < parts.size(); ++pi) {
      const float* src = parts[pi];
      if (!src) continue;
      for (int co = 0; co < Cpart; ++co)
        for (int ci = 0; ci < Cin; ++ci)
          for (int ky = 0; ky < ks; ++ky)
            for (int kx = 0; kx < ks; ++kx) {
              float v;
              if (!flip_t) v = src[(((size_t)co * Cin + ci) * ks + ky) * ks + kx];
              else v = src[(((size_t)ci * Cpart + co) * ks + (ks - 1 - ky)) * ks + (ks - 1 - kx)];
              tmp[((size_t)pi * Cpart + co) * K + (ky * ks + kx) * Cin + ci] = v;
            }
    }
    if (u->bf16) {
      std::vector<uint16_t> b(tmp.size());
      for (size_t i = 0; i < tmp.size(); ++i) b[i] = host_f2bf(tmp[i]);
      return ar.add(b.data(), b.size() * 2);
    }
    return ar.add(tmp.data(), tmp.size() * 4);
  }
  // [Cout][K] bf16 (k = (ky*ks+kx)*Cin + ci) -> MFMA A-fragment order [Cout/32][K/16][64][8]:
  // lane L of k-step s holds W[32*cb + (L & 31)][16*s + 8*(L >> 5) + e] (v_mfma_f32_32x32x16_bf16).
  size_t pack_frag(const float* Wsrc, int Cout, int Cin, int ks) {
    const int K = ks * ks * Cin, nks = K / 16;
    std::vector<uint16_t> b((size_t)Cout * K, 0);
    if (Wsrc)
      for (int cb = 0; cb < Cout / 32; ++cb)
        for (int st = 0; st < nks; ++st)
          for (int L = 0; L < 64; ++L)
            for (int e = 0; e < 8; ++e) {
              const int co = 32 * cb + (L & 31), k = 16 * st + 8 * (L >> 5) + e;
              const int tap = k / Cin, ci = k - tap * Cin, ky = tap / ks, kx = tap - ky * ks;
              b[(((size_t)cb * nks + st) * 64 + L) * 8 + e] =
                  host_f2bf(Wsrc[(((size_t)co * Cin + ci) * ks + ky) * ks + kx]);
            }
    return ar.add(b.data(), b.size() * 2);
  }
  // Phase weights [4][Cout][K] (fp32) in MFMA A-fragment order per phase, [4][Cout/32][K/16][64][8]
  // (conv3x3_gn_p4_kernel's sub-pixel form): lane L of k-step st holds W'[ph][32 cb + L % 32][16 st + 8 (L / 32) + e].
  // SIZE_MAX unless bf16 with Cout % 32 == 0 and K % 16 == 0.
  size_t frag4(const std::vector<float>& tmp, int Cout, int K) {
    if (!u->bf16 || Cout % 32 || K % 16) return SIZE_MAX;
    const int nks = K / 16;
    std::vector<uint16_t> f(tmp.size());
    for (int ph = 0; ph < 4; ++ph)
      for (int cb = 0; cb < Cout / 32; ++cb)
        for (int st = 0; st < nks; ++st)
          for (int L = 0; L < 64; ++L)
            for (int e = 0; e < 8; ++e)
              f[((((size_t)ph * (Cout / 32) + cb) * nks + st) * 64 + L) * 8 + e] =
                  host_f2bf(tmp[((size_t)ph * Cout + 32 * cb + (L & 31)) * K + 16 * st + 8 * (L >> 5) + e]);
    return ar.add(f.data(), f.size() * 2);
  }
  // Nearest-x2 upsample + 3x3 conv (Model.py:123-125) as 4 sub-pixel phases: output
  // (2i+py, 2j+px) sees input rows i+dy+py-1 (dy in {0,1}) with the 3x3 taps folded
  // onto them: W'[ph][co][dy][dx][ci] = sum over ky in R(py,dy), kx in R(px,dx) of
  // W[co][ci][ky][kx], R(0,0)={0}, R(0,1)={1,2}, R(1,0)={0,1}, R(1,1)={2}. Sums in fp64.
  size_t pack_subpix(const float* W, int Cout, int Cin, size_t* wfrag = nullptr) {
    static const int lo[2][2] = {{0, 1}, {0, 2}}, hi[2][2] = {{0, 2}, {1, 2}};  // [p][d] -> k range
    const int K = 4 * Cin;
    std::vector<float> tmp((size_t)4 * Cout * K, 0.f);
    for (int ph = 0; ph < 4; ++ph) {
      const int py = ph >> 1, px = ph & 1;
      for (int co = 0; co < Cout; ++co)
        for (int dy = 0; dy < 2; ++dy)
          for (int dx = 0; dx < 2; ++dx)
            for (int ci = 0; ci < Cin; ++ci) {
              double acc = 0.0;
              for (int ky = lo[py][dy]; ky <= hi[py][dy]; ++ky)
                for (int kx = lo[px][dx]; kx <= hi[px][dx]; ++kx)
                  acc += W ? (double)W[(((size_t)co * Cin + ci) * 3 + ky) * 3 + kx] : 0.0;
              tmp[((size_t)ph * Cout + co) * K + (dy * 2 + dx) * Cin + ci] = (float)acc;
            }
    }
    if (wfrag) *wfrag = frag4(tmp, Cout, K);
    if (u->bf16) {
      std::vector<uint16_t> b(tmp.size());
      for (size_t i = 0; i < tmp.size(); ++i) b[i] = host_f2bf(tmp[i]);
      return ar.add(b.data(), b.size() * 2);
    }
    return ar.add(tmp.data(), tmp.size() * 4);
  }
  // ConvTranspose2d(Cin, Cout, 5, stride 2, padding 2, output_padding 1) (ModelCondition.py:80) as 4
  // sub-pixel phases: output (2m+ry, 2n+rx) = sum over input (m+dy, n+dx), dy, dx in {-1, 0, 1}, of
  // x * w[ci][co][k(ry, dy)][k(rx, dx)] with k(0, d) = 2 - 2d, k(1, d) = 3 - 2d (none for d = -1):
  // W'[ph][co][((dy+1)*3 + dx+1)*Cin + ci] (transposed-conv weight layout [Cin][Cout][5][5])
  // centre_only (a 1x1 input grid, where the d = +-1 taps read only padding): the d = 0 tap alone,
  // W'[ph][co][ci] (K = Cin, ksize 1, pad 0).
  size_t pack_convt_subpix(const float* W, int Cout, int Cin, size_t* wfrag = nullptr, bool centre_only = false) {
    auto kk = [](int r, int d) { return r == 0 ? 2 - 2 * d : (d < 0 ? -1 : 3 - 2 * d); };
    const int rd = centre_only ? 0 : 1, kw = 2 * rd + 1, K = kw * kw * Cin;
    std::vector<float> tmp((size_t)4 * Cout * K, 0.f);
    for (int ph = 0; ph < 4; ++ph) {
      const int ry = ph >> 1, rx = ph & 1;
      for (int co = 0; co < Cout; ++co)
        for (int dy = -rd; dy <= rd; ++dy)
          for (int dx = -rd; dx <= rd; ++dx) {
            const int ky = kk(ry, dy), kx = kk(rx, dx);
            if (ky < 0 || kx < 0 || !W) continue;
            for (int ci = 0; ci < Cin; ++ci)
              tmp[((size_t)ph * Cout + co) * K + ((dy + rd) * kw + dx + rd) * Cin + ci] =
                  W[(((size_t)ci * Cout + co) * 5 + ky) * 5 + kx];
          }
    }
    if (wfrag) *wfrag = frag4(tmp, Cout, K);
    if (u->bf16) {
      std::vector<uint16_t> b(tmp.size());
      for (size_t i = 0; i < tmp.size(); ++i) b[i] = host_f2bf(tmp[i]);
      return ar.add(b.data(), b.size() * 2);
    }
    return ar.add(tmp.data(), tmp.size() * 4);
  }
  int upconv(int s1, const std::string& name, int Cout, int Hout) {
    const Act& A = u->acts[s1];
    const int Cin = A.C, epc = u->bf16 ? 8 : 4;
    // sub-pixel tiles hold whole phase images or lie inside one (128-pixel tiles)
    if (((A.H * A.W) % 128 && 128 % (A.H * A.W)) || Cin % (8 * epc))
      return conv_layer(s1, -1, name, Cout, 3, 1, 1, 1, Hout, Hout);
    const float* W = get(name + ".weight", (int64_t)Cout * Cin * 9);
    size_t wf = SIZE_MAX;
    // fragment-ordered copy for conv3x3_gn_p4_kernel's sub-pixel form (input grids 8x8 / 16x16 / 32x32)
    const bool p4sub = Cout % 128 == 0 && Cin % 64 == 0 && Cin >= 128 && A.H == A.W && (A.W == 8 || A.W == 16 || A.W == 32);
    size_t wt = pack_subpix(W, Cout, Cin, p4sub ? &wf : nullptr);
    size_t b = f32(name + ".bias", Cout);
    int dst = act(Hout, Hout, Cout);
    if (A.H * A.W < 128) u->acts[dst].spi = 4;  // one statistics slot per (image, phase)
    conv(s1, -1, dst, wt, b, Cout, 3, 1, 1, 1);
    Op& o = u->ops.back();
    o.name = name;
    o.subpix = 1;
    o.wfrag = wf;
    return dst;
  }
  size_t concat_f32(const std::vector<const float*>& parts, int n) {
    std::vector<float> tmp((size_t)n * parts.size(), 0.f);
    for (size_t i = 0; i < parts.size(); ++i)
      if (parts[i]) std::memcpy(tmp.data() + i * n, parts[i], n * 4);
    return ar.add(tmp.data(), tmp.size() * 4);
  }
  // W [out][in] -> W^T [in][out] fp32
  size_t transposed(const float* W, int out, int in) {
    std::vector<float> tmp((size_t)out * in, 0.f);
    if (W)
      for (int o = 0; o < out; ++o)
        for (int i = 0; i < in; ++i) tmp[(size_t)i * out + o] = W[(size_t)o * in + i];
    return ar.add(tmp.data(), tmp.size() * 4);
  }

  void gn(int s1, int s2, int dst, const std::string& p, int C, int silu) {
    Op o;
    o.kind = OP_GN;
    o.src1 = s1; o.src2 = s2; o.dst = dst;
    o.gamma = f32(p + ".weight", C);
    o.beta = f32(p + ".bias", C);
    o.silu = silu;
    o.name = p;
    u->ops.push_back(o);
  }
  void conv(int s1, int s2, int dst, size_t wt, size_t bias, int Cout, int ks, int stride, int pad, int ups,
            int temb_col = -1, int resid = -1, int zins = 0) {
    Op o;
    o.kind = OP_CONV;
    o.src1 = s1; o.src2 = s2; o.dst = dst;
    o.wt = wt; o.bias = bias; o.Cout = Cout;
    const int Cin = u->acts[s1].C + (s2 >= 0 ? u->acts[s2].C : 0);
    o.K = ks * ks * Cin;
    o.ksize = ks; o.stride = stride; o.pad = pad; o.upsample = ups; o.zins = zins;
    o.temb_col = temb_col; o.resid = resid;
    u->ops.push_back(o);
  }
  // (Wx / bx: weights [Cout][Cin][ks][ks] and bias built by the caller instead of name's)
  int conv_layer(int s1, int s2, const std::string& name, int Cout, int ks, int stride, int pad, int ups, int Hout,
                 int Wout, int temb_col = -1, int resid = -1, const std::string& gn = "", const float* Wx = nullptr,
                 const float* bx = nullptr) {
    const int Cin = u->acts[s1].C + (s2 >= 0 ? u->acts[s2].C : 0);
    size_t coef = SIZE_MAX;
    if (!gn.empty()) {  // GN coefficient op feeding the fused conv
      Op g;
      g.kind = OP_GNCOEF;
      g.src1 = s1; g.src2 = s2;
      g.gamma = f32(gn + ".weight", Cin);
      g.beta = f32(gn + ".bias", Cin);
      g.coef = coef = ws_off;
      g.name = gn;
      ws_off = (ws_off + (size_t)u->nb_max * Cin * 2 * 4 + 255) & ~(size_t)255;
      u->ops.push_back(g);
    }
    const float* W = Wx ? Wx : get(name + ".weight", (int64_t)Cout * Cin * ks * ks);
    // Taps that read only padding for EVERY output pixel (the 1x1 / 2x2 levels of Arch C: a 3x3
    // conv on a 1x1 image uses its centre tap alone; a stride-2 3x3 / 5x5 conv 2x2 -> 1x1 uses a
    // 2x2 window) are dropped: the conv runs as the ks' x ks' window with pad' = pad - k0.
    // Tap ky is live iff some output row reads an in-range input row:
    // pad - (Hout-1)*stride <= ky <= Hin + pad - 1. Exact (the dropped taps multiply zeros).
    std::vector<float> wwin;
    {
      const Act& A = u->acts[s1];
      const int k0 = std::max(0, pad - (Hout - 1) * stride), k1 = std::min(ks - 1, A.H + pad - 1);
      const int x0 = std::max(0, pad - (Wout - 1) * stride), x1 = std::min(ks - 1, A.W + pad - 1);
      if (itsd::g_tap_prune && gn.empty() && !ups && W && (k0 > 0 || k1 < ks - 1) && k0 == x0 && k1 == x1 && k1 >= k0) {
        const int ks2 = k1 - k0 + 1;
        wwin.resize((size_t)Cout * Cin * ks2 * ks2);
        for (size_t oc = 0; oc < (size_t)Cout * Cin; ++oc)
          for (int ky = 0; ky < ks2; ++ky)
            for (int kx = 0; kx < ks2; ++kx)
              wwin[(oc * ks2 + ky) * ks2 + kx] = W[(oc * ks + k0 + ky) * ks + k0 + kx];
        W = wwin.data();
        ks = ks2;
        pad -= k0;
      }
    }
    size_t wt = pack({W}, Cout, Cin, ks);
    size_t b = bx ? ar.add(bx, (size_t)Cout * 4) : f32(name + ".bias", Cout);
    int dst = act(Hout, Wout, Cout);
    conv(s1, s2, dst, wt, b, Cout, ks, stride, pad, ups, temb_col, resid);
    u->ops.back().name = name;
    u->ops.back().coef = coef;
    if (coef != SIZE_MAX) {  // (the GNCOEF op pushed just before this conv)
      u->ops.back().gn_gamma = u->ops[u->ops.size() - 2].gamma;
      u->ops.back().gn_beta = u->ops[u->ops.size() - 2].beta;
    }
    // (plain 3x3 stride-1 convs too: conv3x3_gn_p4_kernel's plain form, plan_conv's P4_PLAIN)
    const bool plain3 = coef == SIZE_MAX && ks == 3 && stride == 1 && pad == 1 && !ups && Cout % 128 == 0 &&
                        Cin % 128 == 0 && Hout == Wout && (Hout == 32 || Hout == 16 || Hout == 8);
    if ((coef != SIZE_MAX || plain3) && u->bf16 && Cout % 32 == 0 && (ks * ks * Cin) % 16 == 0)
      u->ops.back().wfrag = pack_frag(W, Cout, Cin, ks);
    return dst;
  }
  // conv3x3(silu(GroupNorm(s1 ++ s2))) can run as one fused launch (conv3x3_gn_kernel)
  bool fusable(int s1, int s2, int Cout) const {
    const Act& A = u->acts[s1];
    return u->bf16 && itsd::g_fuse_gn && A.C % 64 == 0 && (s2 < 0 || u->acts[s2].C % 64 == 0) &&
           Cout % 128 == 0 && (conv_gn_eligible(A.H, A.W) || p5_eligible(A.H, A.W));
  }

  int resblock(int x1, int x2, const std::string& p, int in_ch, int out_ch, bool attn) {
    const int H = u->acts[x1].H, W = u->acts[x1].W;
    const int col = u->sumC;
    u->sumC += out_ch;
    temb_cols.push_back({p, (size_t)col});
    // GroupNorm+SiLU either fused into the conv's input staging (conv3x3_gn_kernel) or
    // materialised by gn_apply_kernel
    int h1, o;
    int resid = x1;
    if (fusable(x1, x2, out_ch)) {
      h1 = conv_layer(x1, x2, p + ".block1.2", out_ch, 3, 1, 1, 0, H, W, col, -1, p + ".block1.0");
    } else {
      int g1 = act(H, W, in_ch);
      gn(x1, x2, g1, p + ".block1.0", in_ch, 1);
      h1 = conv_layer(g1, -1, p + ".block1.2", out_ch, 3, 1, 1, 0, H, W, col);
    }
    const bool f2 = fusable(h1, -1, out_ch);
    int g2 = -1;
    if (!f2) {
      g2 = act(H, W, out_ch);
      gn(h1, -1, g2, p + ".block2.0", out_ch, 1);
    }
    int isc = -1;
    if (in_ch != out_ch) {
      resid = conv_layer(x1, x2, p + ".shortcut", out_ch, 1, 1, 0, 0, H, W);
      isc = (int)u->ops.size() - 1;
    }
    if (f2) o = conv_layer(h1, -1, p + ".block2.3", out_ch, 3, 1, 1, 0, H, W, -1, resid, p + ".block2.0");
    else o = conv_layer(g2, -1, p + ".block2.3", out_ch, 3, 1, 1, 0, H, W, -1, resid);
    if (f2 && isc >= 0 && u->bf16 && out_ch % 32 == 0 && u->acts[x1].C % 64 == 0 && (x2 < 0 || u->acts[x2].C % 64 == 0)) {
      // the shortcut as extra K slices of block2 where block2 runs on conv3x3_gn_p5_kernel (run time: conv_args)
      const float* wsc = peek(p + ".shortcut.weight", (int64_t)out_ch * in_ch);
      const float* bsc = peek(p + ".shortcut.bias", out_ch);
      const float* bb2 = peek(p + ".block2.3.bias", out_ch);
      if (wsc && bsc && bb2) {
        std::vector<float> bs((size_t)out_ch);
        for (int c = 0; c < out_ch; ++c) bs[c] = bb2[c] + bsc[c];
        Op& c2 = u->ops.back();
        c2.sc_wfrag = pack_frag(wsc, out_ch, in_ch, 1);
        c2.bias_sc = ar.add(bs.data(), (size_t)out_ch * 4);
        c2.sc_op = isc;
        u->ops[isc].sc_into = (int)u->ops.size() - 1;
      }
    }
    if (attn && H * W == 1 && itsd::g_attn_s1) {
      // AttnBlock over ONE token (ModelCondition.py's 1x1 level; Model.py:145-164): the softmax over a single key
      // is exp(0) / exp(0) = 1 exactly, so h = v and the block is x + proj(v(GN(x))) = x + Wf GN(x) + bf with
      // Wf = Wp Wv, bf = Wp bv + bp (folded here in fp64): one GroupNorm and one 1x1 conv instead of GroupNorm,
      // the q|k|v conv, the attention kernel and the proj conv (q and k never reach the output)
      const std::string a = p + ".attn";
      const int64_t cc = (int64_t)out_ch * out_ch;
      const float* wv = get(a + ".proj_v.weight", cc);
      const float* bv = get(a + ".proj_v.bias", out_ch);
      const float* wp = get(a + ".proj.weight", cc);
      const float* bp = get(a + ".proj.bias", out_ch);
      // (q / k: validated and counted as the reference's keys, never read)
      const bool qk = get(a + ".proj_q.weight", cc) && get(a + ".proj_q.bias", out_ch) && get(a + ".proj_k.weight", cc) &&
                      get(a + ".proj_k.bias", out_ch);
      if (wv && bv && wp && bp && qk) {
        std::vector<float> wf((size_t)cc), bf((size_t)out_ch);
        std::vector<double> row((size_t)out_ch);
        for (int oc = 0; oc < out_ch; ++oc) {
          std::fill(row.begin(), row.end(), 0.0);
          double bacc = (double)bp[oc];
          for (int c = 0; c < out_ch; ++c) {
            const double w = (double)wp[(size_t)oc * out_ch + c];
            const float* vr = wv + (size_t)c * out_ch;
            for (int ic = 0; ic < out_ch; ++ic) row[ic] += w * (double)vr[ic];
            bacc += w * (double)bv[c];
          }
          for (int ic = 0; ic < out_ch; ++ic) wf[(size_t)oc * out_ch + ic] = (float)row[ic];
          bf[oc] = (float)bacc;
        }
        int ga = act(H, W, out_ch);
        gn(o, -1, ga, a + ".group_norm", out_ch, 0);
        const int r = conv_layer(ga, -1, a + ".proj", out_ch, 1, 1, 0, 0, H, W, -1, o, "", wf.data(), bf.data());
        u->ops.back().name = a;
        u->ops.back().tag = ITSD_TAG_ATTN_S1;
        return r;
      }
    }
    if (attn && u->bf16 && itsd::g_attn_fuse && attn_block_ok(H * W, out_ch)) {
      // the whole AttnBlock in one launch (kernels.hip attn_block_kernel). The block is linear on either side of
      // the softmax and its weights are constants, so the four projections fold into two (fp64 here from the fp32
      // weights as loaded, one bf16 rounding in pack_frag):
      //   scores  (h Wq^T + bq)(h Wk^T + bk)^T = (h M + u) h^T + [terms constant along the key axis, which the
      //           softmax over keys cancels exactly],  M = Wq^T Wk, u = Wk^T bq (bk never reaches the output);
      //   output  proj(P v) = P (h W' + b') + bp,  W' = (Wp Wv)^T, b' = Wp bv.
      // As 1x1-conv matrices [Cout][Cin]: Wm[j][i] = sum_a Wk[a][j] Wq[a][i], Wf[o][i] = sum_c Wp[o][c] Wv[c][i].
      const std::string a = p + ".attn";
      const int C = out_ch;
      const int64_t cc = (int64_t)C * C;
      const float* wq = get(a + ".proj_q.weight", cc);
      const float* wk = get(a + ".proj_k.weight", cc);
      const float* wv = get(a + ".proj_v.weight", cc);
      const float* wp = get(a + ".proj.weight", cc);
      const float* bq = get(a + ".proj_q.bias", C);
      const float* bv = get(a + ".proj_v.bias", C);
      get(a + ".proj_k.bias", C);  // (validated and counted as the reference's key, never read)
      std::vector<float> wcat((size_t)2 * cc, 0.f), bcat((size_t)2 * C, 0.f);
      if (wq && wk && wv && wp && bq && bv) {
        std::vector<double> acc((size_t)cc);
        // fold(A, B, ta): acc[r][i] = sum_a (ta ? A[a][r] : A[r][a]) B[a][i]
        auto fold = [&](const float* A, const float* B, bool ta, float* dst) {
          std::fill(acc.begin(), acc.end(), 0.0);
          for (int r = 0; r < C; ++r) {
            double* row = acc.data() + (size_t)r * C;
            for (int k = 0; k < C; ++k) {
              const double w = (double)(ta ? A[(size_t)k * C + r] : A[(size_t)r * C + k]);
              const float* br = B + (size_t)k * C;
              for (int i = 0; i < C; ++i) row[i] += w * (double)br[i];
            }
          }
          for (int64_t i = 0; i < cc; ++i) dst[i] = (float)acc[i];
        };
        fold(wk, wq, true, wcat.data());        // M rows: Wk^T Wq
        fold(wp, wv, false, wcat.data() + cc);  // W' rows: Wp Wv
        for (int j = 0; j < C; ++j) {
          double su = 0.0, sb = 0.0;
          for (int k = 0; k < C; ++k) {
            su += (double)wk[(size_t)k * C + j] * (double)bq[k];
            sb += (double)wp[(size_t)j * C + k] * (double)bv[k];
          }
          bcat[j] = (float)su;
          bcat[C + j] = (float)sb;
        }
      }
      Op ab;
      ab.kind = OP_ATTNBLOCK;
      ab.src1 = o;
      ab.gamma = f32(a + ".group_norm.weight", out_ch);
      ab.beta = f32(a + ".group_norm.bias", out_ch);
      ab.wt = pack_frag(wcat.data(), 2 * out_ch, out_ch, 1);  // [M rows | W' rows]
      ab.bias = ar.add(bcat.data(), bcat.size() * 4);          // [u | b']
      ab.bias2 = f32(a + ".proj.bias", out_ch);
      ab.S = H * W;
      ab.C = out_ch;
      ab.dst = act(H, W, out_ch);
      ab.name = a;
      ab.tag = ITSD_TAG_ATTNBLOCK;
      u->ops.push_back(ab);
      return ab.dst;
    }
    if (attn) {
      const std::string a = p + ".attn";
      int ga = act(H, W, out_ch);
      gn(o, -1, ga, a + ".group_norm", out_ch, 0);
      const int64_t cc = (int64_t)out_ch * out_ch;
      size_t wqkv = pack({get(a + ".proj_q.weight", cc), get(a + ".proj_k.weight", cc), get(a + ".proj_v.weight", cc)},
                         out_ch, out_ch, 1);
      size_t bqkv = concat_f32({get(a + ".proj_q.bias", out_ch), get(a + ".proj_k.bias", out_ch),
                                get(a + ".proj_v.bias", out_ch)}, out_ch);
      int qkv = act(H, W, 3 * out_ch);
      conv(ga, -1, qkv, wqkv, bqkv, 3 * out_ch, 1, 1, 0, 0);
      u->ops.back().name = a;
      u->ops.back().tag = ITSD_TAG_QKV;
      // MFMA attention (bf16): V goes channel-major to its own buffer from the conv epilogue
      const int S = H * W;
      int vt = -1;
      // (S <= 256: whole-row MFMA kernel; longer sequences: flash kernel, C <= 256)
      if (u->bf16 && S % 16 == 0 && out_ch % 64 == 0 && (S <= 256 || attn_flash_ok(S, out_ch) || attn_cs_ok(S, out_ch))) {
        vt = act(out_ch, S, 1);
        u->ops.back().vt = vt;
        u->ops.back().vt_from = 2 * out_ch;
      }
      int ao = act(H, W, out_ch);
      Op at;
      at.kind = OP_ATTN;
      at.name = a;
      at.src1 = qkv; at.dst = ao; at.S = H * W; at.C = out_ch; at.vt = vt;
      u->ops.push_back(at);
      o = conv_layer(ao, -1, a + ".proj", out_ch, 1, 1, 0, 0, H, W, -1, o);
    }
    return o;
  }
};

int build(itsd_unet* u, const itsd_tensor_view* views, int nviews) {
  Builder b;
  b.u = u;
  for (int i = 0; i < nviews; ++i) b.w[views[i].name] = {views[i].data, views[i].numel};
  const itsd_unet_desc& d = u->d;
  const int ch = d.ch, tdim = 4 * ch, H = d.img_size;
  u->ch = ch; u->tdim = tdim; u->H = H;

  // embeddings
  if (!u->cfg) {
    u->freq = b.f32("time_embedding.freq_coeffs", ch / 2);
    u->W0t = b.transposed(b.get("time_embedding.timembedding.0.weight", (int64_t)tdim * ch), tdim, ch);
    u->b0 = b.f32("time_embedding.timembedding.0.bias", tdim);
    u->W2t = b.transposed(b.get("time_embedding.timembedding.2.weight", (int64_t)tdim * tdim), tdim, tdim);
    u->b2 = b.f32("time_embedding.timembedding.2.bias", tdim);
  } else {
    u->ttable = b.f32("time_embedding.timembedding.0.weight", (int64_t)d.T * ch);
    u->W0t = b.transposed(b.get("time_embedding.timembedding.1.weight", (int64_t)tdim * ch), tdim, ch);
    u->b0 = b.f32("time_embedding.timembedding.1.bias", tdim);
    u->W2t = b.transposed(b.get("time_embedding.timembedding.3.weight", (int64_t)tdim * tdim), tdim, tdim);
    u->b2 = b.f32("time_embedding.timembedding.3.bias", tdim);
    u->ctable = b.f32("cond_embedding.condEmbedding.0.weight", (int64_t)(d.num_labels + 1) * ch);
    u->C1t = b.transposed(b.get("cond_embedding.condEmbedding.1.weight", (int64_t)tdim * ch), tdim, ch);
    u->cb1 = b.f32("cond_embedding.condEmbedding.1.bias", tdim);
    u->C3t = b.transposed(b.get("cond_embedding.condEmbedding.3.weight", (int64_t)tdim * tdim), tdim, tdim);
    u->cb3 = b.f32("cond_embedding.condEmbedding.3.bias", tdim);
  }
  u->head_w = b.f32("head.weight", (int64_t)ch * 27);
  u->head_b = b.f32("head.bias", ch);
  u->head_out = b.act(H, H, ch);
  // (head_mfma_kernel: 128-pixel tiles of whole rows, couts in 32-blocks; else the plain head kernel)
  if (u->bf16 && itsd::g_io_mfma && ch % 32 == 0 && (H * H) % 128 == 0 && 128 % H == 0) {
    // [Cout][32] bf16, k = ci*9 + tap (the reference's flat per-cout order), zero-padded
    const float* hw = b.peek("head.weight", (int64_t)ch * 27);
    if (hw) {
      std::vector<uint16_t> wm((size_t)ch * 32, 0);
      for (int co = 0; co < ch; ++co)
        for (int k = 0; k < 27; ++k) wm[(size_t)co * 32 + k] = host_f2bf(hw[(size_t)co * 27 + k]);
      u->head_wmf = b.ar.add(wm.data(), wm.size() * 2);
    }
  } else {
    // the plain head kernel's blocks are one statistics slot of whole rows, or a segment of one row (launch_head):
    // refused here, not at the first forward
    const int G = stat_slot_px(H * H);
    if ((H * H) % G || (G % H && H % G))
      return fail(ITSD_ERR_INVALID, "img_size " + std::to_string(H) + " not supported by the head kernel (its " +
                                        std::to_string(G) + "-pixel blocks hold whole rows or lie inside one)");
  }

  std::vector<int> hs{u->head_out};
  int cur = u->head_out;
  int now = ch;
  int ndown = 0;
  auto P = [](const char* s, int i) { return std::string(s) + "." + std::to_string(i); };
  for (int i = 0; i < d.n_mult; ++i) {
    const int out = ch * d.ch_mult[i];
    bool at = false;
    for (int k = 0; k < d.n_attn; ++k) at |= (d.attn[k] == i);
    if (u->cfg) at = true;
    for (int r = 0; r < d.num_res_blocks; ++r) {
      cur = b.resblock(cur, -1, P("downblocks", ndown++), now, out, at);
      now = out;
      hs.push_back(cur);
    }
    if (i != d.n_mult - 1) {
      const std::string p = P("downblocks", ndown++);
      const int Hc = b.u->acts[cur].H;
      if (!u->cfg) {
        cur = b.conv_layer(cur, -1, p + ".main", now, 3, 2, 1, 0, Hc / 2, Hc / 2);
      } else if (!itsd::g_down_merge) {  // c1(x) + c2(x), ModelCondition.py:71-73, as two convs
        int t1 = b.conv_layer(cur, -1, p + ".c1", now, 3, 2, 1, 0, Hc / 2, Hc / 2);
        cur = b.conv_layer(cur, -1, p + ".c2", now, 5, 2, 2, 0, Hc / 2, Hc / 2, -1, t1);
      } else {  // c1(x) + c2(x), ModelCondition.py:71-73: both stride 2 and centred on the same input
        // pixel (3x3 pad 1, 5x5 pad 2), so the sum is ONE 5x5 conv with c1's taps added onto c2's
        // inner 3x3 (summed in fp32 before packing) and bias b1 + b2: 25 Cin of K instead of 34 Cin,
        // one launch and no intermediate tensor
        const int Cin = b.u->acts[cur].C;
        const float* W1 = b.get(p + ".c1.weight", (int64_t)now * Cin * 9);
        const float* W2 = b.get(p + ".c2.weight", (int64_t)now * Cin * 25);
        const float* b1 = b.get(p + ".c1.bias", now);
        const float* b2 = b.get(p + ".c2.bias", now);
        std::vector<float> wm((size_t)now * Cin * 25, 0.f), bm(now, 0.f);
        if (W2) std::memcpy(wm.data(), W2, wm.size() * 4);
        if (W1)
          for (size_t oc = 0; oc < (size_t)now * Cin; ++oc)
            for (int ky = 0; ky < 3; ++ky)
              for (int kx = 0; kx < 3; ++kx) wm[(oc * 5 + ky + 1) * 5 + kx + 1] += W1[(oc * 3 + ky) * 3 + kx];
        for (int c = 0; c < now; ++c) bm[c] = (b1 ? b1[c] : 0.f) + (b2 ? b2[c] : 0.f);
        cur = b.conv_layer(cur, -1, p + ".c12", now, 5, 2, 2, 0, Hc / 2, Hc / 2, -1, -1, "", wm.data(), bm.data());
        u->ops.back().name = p;
        u->ops.back().tag = ITSD_TAG_DOWN_MERGE;
      }
      hs.push_back(cur);
    }
  }
  cur = b.resblock(cur, -1, "middleblocks.0", now, now, true);
  cur = b.resblock(cur, -1, "middleblocks.1", now, now, false);
  int nup = 0;
  for (int i = d.n_mult - 1; i >= 0; --i) {
    const int out = ch * d.ch_mult[i];
    bool at = false;
    for (int k = 0; k < d.n_attn; ++k) at |= (d.attn[k] == i);
    if (u->cfg) at = false;
    for (int r = 0; r < d.num_res_blocks + 1; ++r) {
      int skip = hs.back();
      hs.pop_back();
      cur = b.resblock(cur, skip, P("upblocks", nup++), now + u->acts[skip].C, out, at);
      now = out;
    }
    if (i != 0) {
      const std::string p = P("upblocks", nup++);
      const int Hc = b.u->acts[cur].H;
      if (!u->cfg) {
        cur = b.upconv(cur, p + ".main", now, 2 * Hc);
      } else {  // ConvTranspose2d(5, 2, 2, 1) then Conv 3x3, ModelCondition.py:83-85
        const float* Wt = b.get(p + ".t.weight", (int64_t)now * now * 25);
        size_t bt = b.f32(p + ".t.bias", now);
        int tmp = b.act(2 * Hc, 2 * Hc, now);
        const int epc = u->bf16 ? 8 : 4;
        if (((Hc * Hc) % 128 == 0 || 128 % (Hc * Hc) == 0) && now % (8 * epc) == 0) {
          // sub-pixel form: 4 phase-wise 3x3 convs over the input grid (9 of the 25 taps a phase,
          // against 25 per output of the zero-insertion form)
          // (+ the fragment-ordered phase weights for conv3x3_gn_p4_kernel's sub-pixel form at 8x8 .. 32x32 inputs)
          size_t wf = SIZE_MAX;
          const bool p4sub = now % 128 == 0 && now >= 128 && (Hc == 8 || Hc == 16 || Hc == 32);
          // (a 1x1 input grid: the centre tap alone, K = Cin instead of 9 Cin)
          const bool c1 = Hc == 1 && itsd::g_tap_prune;
          size_t wt = b.pack_convt_subpix(Wt, now, now, p4sub ? &wf : nullptr, c1);
          if (Hc * Hc < 128) u->acts[tmp].spi = 4;  // one statistics slot per (image, phase)
          b.conv(cur, -1, tmp, wt, bt, now, c1 ? 1 : 3, 1, c1 ? 0 : 1, 0);
          u->ops.back().subpix = 2;
          u->ops.back().wfrag = wf;
          u->ops.back().name = p + ".t";
          u->ops.back().tag = ITSD_TAG_CONVT;
        } else {
          size_t wt = b.pack({Wt}, now, now, 5, true);
          b.conv(cur, -1, tmp, wt, bt, now, 5, 1, 2, 0, -1, -1, 1);
          u->ops.back().name = p + ".t";
          u->ops.back().tag = ITSD_TAG_CONVT;
        }
        cur = b.conv_layer(tmp, -1, p + ".c", now, 3, 1, 1, 0, 2 * Hc, 2 * Hc);
      }
    }
  }
  if (!hs.empty()) return fail(ITSD_ERR_INVALID, "internal: skip stack not empty");
  u->tail_in = cur;
  u->tail_gn_g = b.f32("tail.0.weight", now);
  u->tail_gn_b = b.f32("tail.0.bias", now);
  u->tail_w = b.f32("tail.2.weight", (int64_t)3 * now * 9);
  u->tail_b = b.f32("tail.2.bias", 3);
  if (u->bf16 && itsd::g_io_mfma && tail_mfma_ok(H, H, now)) {
    // GroupNorm+SiLU fused into the MFMA tail: coefficients instead of a normalised copy;
    // weights as [9C/32 k-steps][4 lane groups][3 couts][8 k] bf16, k = tap*C + ci
    const float* tw = b.peek("tail.2.weight", (int64_t)3 * now * 9);
    if (tw) {
      const int nks = 9 * now / 32;
      std::vector<uint16_t> wm((size_t)nks * 4 * 3 * 8);
      for (int ks = 0; ks < nks; ++ks)
        for (int kg = 0; kg < 4; ++kg)
          for (int co = 0; co < 3; ++co)
            for (int j = 0; j < 8; ++j) {
              const int k = 32 * ks + 8 * kg + j, tap = k / now, ci = k - tap * now;
              wm[(((size_t)ks * 4 + kg) * 3 + co) * 8 + j] = host_f2bf(tw[((size_t)co * now + ci) * 9 + tap]);
            }
      u->tail_wmf = b.ar.add(wm.data(), wm.size() * 2);
    }
    u->tail_coef = b.ws_off;
    b.ws_off = (b.ws_off + (size_t)u->nb_max * now * 2 * 4 + 255) & ~(size_t)255;
  } else {
    u->tail_g = b.act(H, H, now);
  }

  // all ResBlock temb_proj (and cond_proj) Linears as one [tdim][sumC] matrix
  {
    std::vector<float> Wp((size_t)u->sumC * tdim), bpv(u->sumC), Wc, bcv;
    if (u->cfg) { Wc.resize(Wp.size()); bcv.resize(u->sumC); }
    for (size_t k = 0; k < b.temb_cols.size(); ++k) {
      const std::string& p = b.temb_cols[k].first;
      const size_t col = b.temb_cols[k].second;
      const size_t next = (k + 1 < b.temb_cols.size()) ? b.temb_cols[k + 1].second : (size_t)u->sumC;
      const int oc = (int)(next - col);
      auto fill = [&](const std::string& nm, std::vector<float>& Wd, std::vector<float>& bd) {
        const float* W = b.get(nm + ".weight", (int64_t)oc * tdim);
        const float* bb = b.get(nm + ".bias", oc);
        if (!W || !bb) return;
        for (int o = 0; o < oc; ++o) {
          for (int i = 0; i < tdim; ++i) Wd[(size_t)i * u->sumC + col + o] = W[(size_t)o * tdim + i];
          bd[col + o] = bb[o];
        }
      };
      fill(p + ".temb_proj.1", Wp, bpv);
      if (u->cfg) fill(p + ".cond_proj.1", Wc, bcv);
    }
    u->Wpt = b.ar.add(Wp.data(), Wp.size() * 4);
    u->bp = b.ar.add(bpv.data(), bpv.size() * 4);
    if (u->cfg) {
      u->Wct = b.ar.add(Wc.data(), Wc.size() * 4);
      u->bc = b.ar.add(bcv.data(), bcv.size() * 4);
    }
  }
  if (!b.err.empty()) return fail(ITSD_ERR_WEIGHTS, b.err);
  if ((int)b.used != nviews) {
    return fail(ITSD_ERR_WEIGHTS, "state_dict has " + std::to_string(nviews) + " entries, model uses " +
                                      std::to_string(b.used) + " (unexpected keys present)");
  }
  // a GroupNorm op over the output of the conv right before it (and nothing else): a candidate for conv_small's fused
  // GroupNorm output (conv_args decides per launch; every activation has its own buffer, so the GroupNorm's output
  // never aliases the conv's operands)
  for (size_t i = 1; i < u->ops.size(); ++i) {
    Op& g = u->ops[i];
    Op& p = u->ops[i - 1];
    if (g.kind == OP_GN && g.src2 < 0 && p.kind == OP_CONV && p.dst == g.src1 && p.sc_into < 0 && p.vt < 0) {
      p.gn_next = (int)i;
      g.gn_from = (int)i - 1;
    }
  }
  // channel-statistics slabs for every tensor a GroupNorm reads (written by its producer)
  {
    std::vector<int> need;
    for (const Op& o : u->ops)
      if (o.kind == OP_GN || o.kind == OP_GNCOEF || o.kind == OP_ATTNBLOCK) {
        need.push_back(o.src1);
        if (o.src2 >= 0) need.push_back(o.src2);
      }
    need.push_back(u->tail_in);
    for (int id : need) {
      Act& A = u->acts[id];
      if (A.stats != SIZE_MAX) continue;
      const int HW = A.H * A.W;
      if (!(128 % HW == 0 || HW % 128 == 0))
        return fail(ITSD_ERR_INVALID, "spatial size " + std::to_string(HW) + " not supported by the GN statistics slots");
      const size_t slots = (size_t)u->nb_max * stat_spi(HW, A.spi);
      A.stats = b.ws_off;
      b.ws_off = (b.ws_off + slots * 2 * A.C * 4 + 255) & ~(size_t)255;
      bool produced = (id == u->head_out);
      for (const Op& o : u->ops) produced |= ((o.kind == OP_CONV || o.kind == OP_ATTNBLOCK) && o.dst == id);
      if (!produced) return fail(ITSD_ERR_INVALID, "internal: GroupNorm input without a statistics producer");
    }
  }
  // device arenas
  HIPCHK(hipMalloc(&u->wdev, b.ar.host.size()));
  HIPCHK(hipMemcpy(u->wdev, b.ar.host.data(), b.ar.host.size(), hipMemcpyHostToDevice));
  u->ws_bytes = b.ws_off;
  HIPCHK(hipMalloc(&u->ws, u->ws_bytes));
  return ITSD_OK;
}

// ------------------------------------------------------------------------- program execution
struct RunCtx {
  int nb;                // images in the UNet batch
  const float* x;        // head input NCHW
  int x_mod;             // head reads x[img % x_mod]
  const float* temb;     // temb rows/table base
  const int* tsel;       // device t (table mode) or null
  long long temb_img_stride;
  const int32_t* labels; // CFG labels
  int label_mod;
  int uncond_from;
  TailArgs tail;
  // census
  bool census = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>>* evs = nullptr;
  std::vector<int>* ev_kind = nullptr;
  std::vector<double>* ev_flops = nullptr;
  std::vector<int>* ev_kid = nullptr;  // kernel_id of the op's first launch (itsd_kernel_name)
  std::vector<int>* ev_op = nullptr;   // program op index (1-based; 0 = head / tail) of each launch
};

// The launch arguments and the launch plan of a conv op (resolve_program calls it once per op and pass). Every failure
// returns before a fold is set: a failed op's arguments fold nothing.
int conv_args(itsd_unet* u, const Op& o, const RunCtx& c, ConvArgs& a, ConvPlan& p) {
    const Act& in = u->acts[o.src1];
    const Act& out = u->acts[o.dst];
    a.src1 = u->ap(o.src1);
    a.src2 = o.src2 >= 0 ? u->ap(o.src2) : nullptr;
    a.C1 = in.C;
    a.C2 = o.src2 >= 0 ? u->acts[o.src2].C : 0;
    a.Hin = in.H; a.Win = in.W; a.Hout = out.H; a.Wout = out.W;
    a.ksize = o.ksize; a.stride = o.stride; a.pad = o.pad; a.upsample = o.upsample;
    a.wt = u->wdev + o.wt;
    a.wfrag = o.wfrag != SIZE_MAX ? u->wdev + o.wfrag : nullptr;
    a.Cout = o.Cout; a.K = o.K;
    a.bias = u->wp(o.bias);
    if (o.temb_col >= 0) {
      a.temb = c.temb + o.temb_col;
      a.temb_tsel = c.tsel;
      a.temb_row_stride = u->sumC;
      a.temb_img_stride = c.temb_img_stride;
      if (u->cfg) {
        a.cemb = u->cemb_table + o.temb_col;
        a.cemb_labels = (const int*)c.labels;
        a.cemb_row_stride = u->sumC;
        a.cemb_label_mod = c.label_mod;
        a.cemb_uncond_from = c.uncond_from;
      }
    }
    a.resid = o.resid >= 0 ? u->ap(o.resid) : nullptr;
    a.out = u->ap(o.dst);
    a.M = c.nb * out.H * out.W;
    a.stats = out.stats != SIZE_MAX ? (float*)(u->ws + out.stats) : nullptr;
    a.zero = u->zero_page;
    a.splitk_ws = u->splitk_ws;
    a.splitk_cap = itsd_unet::kSplitkCap;
    a.tickets = u->tickets;
    a.err = u->d_nan + 1;
    a.spin_bound = itsd::g_spin_bound;
    if (o.vt >= 0) {
      if (o.vt_from % 128 || (out.H * out.W) % 8) return fail(ITSD_ERR_INVALID, "internal: bad channel-major V split");
      a.vt_out = u->ap(o.vt);
      a.vt_from = o.vt_from;
    }
    a.zins = o.zins;
    a.dbg = itsd::g_conv_dbg;
    a.xcd = itsd::g_p4_xcd == 1 || (itsd::g_p4_xcd == 2 && a.Wout == 8);
    if (o.subpix) {  // input-grid GEMM with 2x2 (upsample) / 3x3 (ConvTranspose2d) taps per phase (conv.hip)
      a.subpix = o.subpix;
      a.Hout = in.H; a.Wout = in.W;
      a.M = c.nb * in.H * in.W;
      a.ksize = o.subpix == 2 ? o.ksize : 2; a.pad = o.subpix == 2 ? o.pad : 0; a.upsample = 0; a.zins = 0;
      a.K = a.ksize * a.ksize * (a.C1 + a.C2);
      a.tap_live = o.subpix == 2 && a.ksize == 3 && itsd::g_convt_prune;  // (p4: skip the zero taps)
    }
    if (o.coef != SIZE_MAX) {
      if (!u->bf16 || o.ksize != 3 || o.stride != 1 || o.pad != 1 || o.upsample || o.zins ||
          !(conv_gn_eligible(in.H, in.W) || p5_eligible(in.H, in.W)) || a.C1 % 64 || a.C2 % 64 || a.Cout % 128)
        return fail(ITSD_ERR_INVALID, "internal: fused GroupNorm conv on an unsupported shape");
      a.gn_coef = (const float*)(u->ws + o.coef);
    }
    {  // the kernel moves 16-B chunks: every chunk must sit inside one source and one tap
      const int epc = u->bf16 ? 8 : 4;
      if (a.C1 % epc || a.C2 % epc || a.Cout % 4 || a.K % epc)
        return fail(ITSD_ERR_INVALID, "conv channels must be multiples of " + std::to_string(epc));
    }
  // The launch plan, made once here: launch_conv runs it, and the three folds below are read off it (none of the
  // fields they set enters the plan). A block2 conv offers its ResBlock's 1x1 shortcut as a candidate.
  if (o.sc_op >= 0 && itsd::g_p5_sc) {
    const Op& sc = u->ops[o.sc_op];
    a.sc_src1 = u->ap(sc.src1);
    a.sc_src2 = sc.src2 >= 0 ? u->ap(sc.src2) : nullptr;
    a.sc_C1 = u->acts[sc.src1].C;
    a.sc_C2 = sc.src2 >= 0 ? u->acts[sc.src2].C : 0;
    a.sc_wfrag = u->wdev + o.sc_wfrag;
  }
  p = plan_conv(a, u->bf16);
  const bool p5 = p.kernel == ConvKernel::P5 || p.kernel == ConvKernel::P5_SHARED;
  const bool p4 = p.kernel == ConvKernel::P4_GN || p.kernel == ConvKernel::P4_C96;
  if (p.sc_split) {  // the shortcut folded in as K slices (run_program then skips the shortcut's launch)
    a.bias = u->wp(o.bias_sc);
    a.resid = nullptr;
  } else {
    a.sc_src1 = a.sc_src2 = a.sc_wfrag = nullptr;
    a.sc_C1 = a.sc_C2 = 0;
  }
  // gn_fold: conv3x3_gn_p5_kernel / conv3x3_gn_p4_kernel reduce the input's statistics slabs themselves
  // (run_program then skips the op's gn_coef launch); up to 8 slots an image (32x32): the 32 slots of a
  // 64x64 image made the in-kernel reduction 4-12 dependent load batches (measured: the 64x64 level
  // 0.90 ms folded vs 0.55 ms with its gn_coef launches, C4 at N = 16)
  if (a.gn_coef && o.gn_gamma != SIZE_MAX && itsd::g_gn_fold && (a.C1 + a.C2) % 128 == 0 && in.H * in.W <= 1024 &&
      (p5 || p4)) {
    a.gn_fold = 1;
    a.gn_st1 = (const float*)(u->ws + u->acts[o.src1].stats);
    a.gn_st2 = o.src2 >= 0 ? (const float*)(u->ws + u->acts[o.src2].stats) : nullptr;
    a.gn_spi1 = u->acts[o.src1].spi;
    a.gn_spi2 = o.src2 >= 0 ? u->acts[o.src2].spi : 0;
    a.gn_gamma = u->wp(o.gn_gamma);
    a.gn_beta = u->wp(o.gn_beta);
  }
  // (round 6) the consumer GroupNorm(+SiLU) in conv_small's epilogue (run_program then skips the GN op): whole-image
  // tiles with one statistics slot an image (HWo <= 16: the CFG model's 2x2 / 1x1 levels), a group's gs = Cout / 32
  // channels inside one 64-cout tile
  if (o.gn_next >= 0 && itsd::g_small_gn && u->bf16 && a.stats && !a.gn_coef && !o.subpix && !a.vt_out &&
      u->acts[o.dst].spi == 0) {
    const int HWo = a.Hout * a.Wout, gs = a.Cout / kGnGroups;
    if (HWo <= 16 && 64 % HWo == 0 && a.Cout % 64 == 0 && gs >= 2 && 64 % gs == 0 && p.kernel == ConvKernel::SMALL) {
      const Op& g = u->ops[o.gn_next];
      a.gn_out = u->ap(g.dst);
      a.go_gamma = u->wp(g.gamma);
      a.go_beta = u->wp(g.beta);
      a.go_silu = g.silu;
    }
  }
  return ITSD_OK;
}

// A conv op resolved for one pass: its launch arguments, its plan, and conv_args' status (with its message) for when
// the op's turn comes. Non-conv ops keep the empty entry.
struct ConvLaunch {
  ConvArgs a{};
  ConvPlan p;
  int rc = ITSD_OK;
  std::string err;
};

// Every conv op of the program resolved once (indexed as u->ops): what run_program launches, skips and reports.
std::vector<ConvLaunch> resolve_program(itsd_unet* u, const RunCtx& c) {
  std::vector<ConvLaunch> r(u->ops.size());
  for (size_t oi = 0; oi < u->ops.size(); ++oi) {
    if (u->ops[oi].kind != OP_CONV) continue;
    r[oi].rc = conv_args(u, u->ops[oi], c, r[oi].a, r[oi].p);
    if (r[oi].rc != ITSD_OK) r[oi].err = g_err;
  }
  return r;
}

// The op (index in u->ops) whose launch does op oi's work, or -1 where op oi is launched itself: what run_program
// skips and itsd_unet_op_info reports. A conv whose conv_args failed folds nothing and fails at its turn.
int folded_into(const itsd_unet* u, const std::vector<ConvLaunch>& rp, size_t oi) {
  const Op& o = u->ops[oi];
  // gn_fold: the consumer conv finalizes this GroupNorm itself
  if (o.kind == OP_GNCOEF && oi + 1 < u->ops.size() && rp[oi + 1].a.gn_fold) return (int)oi + 1;
  // a GroupNorm its producer conv wrote in its epilogue
  if (o.kind == OP_GN && o.gn_from >= 0 && rp[o.gn_from].a.gn_out) return o.gn_from;
  // a shortcut its block2 conv runs as K slices
  if (o.kind == OP_CONV && o.sc_into >= 0 && rp[o.sc_into].p.sc_split) return o.sc_into;
  return -1;
}

// What both GroupNorm op kinds read: the (concatenated) input's channels, its statistics slabs, gamma / beta.
GNArgs gn_args(const itsd_unet* u, const Op& o) {
  GNArgs g{};
  g.C1 = u->acts[o.src1].C;
  g.C2 = o.src2 >= 0 ? u->acts[o.src2].C : 0;
  g.HW = u->acts[o.src1].H * u->acts[o.src1].W;
  g.gamma = u->wp(o.gamma);
  g.beta = u->wp(o.beta);
  g.eps = kGnEps;
  g.st1 = (const float*)(u->ws + u->acts[o.src1].stats);
  g.st2 = o.src2 >= 0 ? (const float*)(u->ws + u->acts[o.src2].stats) : nullptr;
  g.spi1 = u->acts[o.src1].spi;
  g.spi2 = o.src2 >= 0 ? u->acts[o.src2].spi : 0;
  return g;
}

// cl: the op's resolved entry (conv ops)
int launch_op(itsd_unet* u, const Op& o, const RunCtx& c, const ConvLaunch* cl, hipStream_t s) {
  hipError_t e = hipSuccess;
  if (o.kind == OP_GNCOEF) {
    e = launch_gn_coef(gn_args(u, o), c.nb, (float*)(u->ws + o.coef), s);
  } else if (o.kind == OP_GN) {
    GNArgs a = gn_args(u, o);
    a.src1 = u->ap(o.src1);
    a.src2 = o.src2 >= 0 ? u->ap(o.src2) : nullptr;
    a.silu = o.silu;
    a.dst = u->ap(o.dst);
    e = u->bf16 ? launch_groupnorm<bf16_t>(a, c.nb, s) : launch_groupnorm<float>(a, c.nb, s);
  } else if (o.kind == OP_CONV) {
    if (cl->rc != ITSD_OK) return fail(cl->rc, cl->err);
    e = u->bf16 ? launch_conv<bf16_t>(cl->a, cl->p, s) : launch_conv<float>(cl->a, cl->p, s);
  } else if (o.kind == OP_ATTNBLOCK) {
    AttnBlockArgs a{};
    const Act& in = u->acts[o.src1];
    const Act& out = u->acts[o.dst];
    a.x = (const bf16_t*)u->ap(o.src1);
    a.st = (const float*)(u->ws + in.stats);
    a.spi = stat_spi(in.H * in.W, in.spi);
    a.gamma = u->wp(o.gamma);
    a.beta = u->wp(o.beta);
    a.wmv = (const bf16_t*)(u->wdev + o.wt);
    a.buv = u->wp(o.bias);
    a.bp = u->wp(o.bias2);
    a.out = (bf16_t*)u->ap(o.dst);
    a.out_stats = out.stats != SIZE_MAX ? (float*)(u->ws + out.stats) : nullptr;
    a.scale = (float)std::pow((double)o.C, -0.5);
    a.n = c.nb;
    a.S = o.S;
    // attn_block_split_kernel's partial-score slab in the split-K workspace (ops run in stream order; <= 4 MB
    // at n * G <= 256)
    static_assert((4ll << 20) / 4 <= itsd_unet::kSplitkCap, "the partial-score slab fits the split-K workspace");
    a.spart = u->splitk_ws;
    a.sync = u->attn_sync;
    a.err = u->d_nan + 1;
    a.spin_bound = itsd::g_spin_bound;
    e = launch_attn_block(a, o.C, s);
  } else {
    AttnArgs a{};
    a.qkv = u->ap(o.src1);
    a.vt = o.vt >= 0 ? u->ap(o.vt) : nullptr;
    a.out = u->ap(o.dst);
    a.S = o.S; a.C = o.C;
    a.scale = (float)std::pow((double)o.C, -0.5);
    e = u->bf16 ? launch_attn<bf16_t>(a, c.nb, s) : launch_attn<float>(a, c.nb, s);
  }
  if (e != hipSuccess) return fail(ITSD_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
  return ITSD_OK;
}

double op_flops(const itsd_unet* u, const Op& o, int nb) {
  if (o.kind == OP_CONV) {  // executed MFMA work (sub-pixel upsample convs: 4 of the 9 taps)
    const Act& out = u->acts[o.dst];
    // (executed: nearest-x2 upsample convs 4 of their 9 taps per output; the sub-pixel ConvTranspose2d's
    // K is already its 9 taps per output)
    return 2.0 * nb * out.H * out.W * (double)o.Cout * (o.subpix == 1 ? o.K * 4 / 9 : o.K);
  }
  if (o.kind == OP_ATTN) return 2.0 * 2.0 * nb * (double)o.S * o.S * o.C;
  if (o.kind == OP_ATTNBLOCK)  // the algorithmic count: q|k|v and proj projections + the two attention products (the
    // folded kernel executes two C x C projections, not four: 2 S (2 C^2) + 2 * 2 S^2 C an image)
    return 2.0 * nb * (double)o.S * (4.0 * o.C * o.C) + 2.0 * 2.0 * nb * (double)o.S * o.S * o.C;
  return 0.0;
}

// rp: resolve_program's entries for this pass
int run_program(itsd_unet* u, const RunCtx& c, const std::vector<ConvLaunch>& rp, hipStream_t s) {
  int cur_op = 0;  // program op being launched (census: 1-based, 0 head / tail)
  auto mark = [&](int kind, double fl, const std::function<int()>& fn) -> int {
    if (!c.census) return fn();
    if (c.ev_op) c.ev_op->push_back(cur_op);
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a));
    if (hipError_t e = hipEventCreate(&b); e != hipSuccess) {
      hipEventDestroy(a);
      return fail(ITSD_ERR_HIP, std::string("hipEventCreate(&b): ") + hipGetErrorString(e));
    }
    HIPCHK(hipEventRecord(a, s));
    itsd::g_last_kernel = nullptr;
    int r = fn();
    HIPCHK(hipEventRecord(b, s));
    c.evs->push_back({a, b});
    c.ev_kind->push_back(kind);
    c.ev_flops->push_back(fl);
    if (c.ev_kid) c.ev_kid->push_back(itsd::kernel_id(itsd::g_last_kernel));
    return r;
  };
  // head
  CHK(mark(-1, 2.0 * c.nb * u->H * u->H * 27.0 * u->ch, [&]() -> int {
    HeadArgs h{};
    h.x = c.x;
    h.w = u->wp(u->head_w);
    h.b = u->wp(u->head_b);
    h.out = u->ap(u->head_out);
    h.H = u->H; h.W = u->H; h.Cout = u->ch; h.n = c.nb; h.x_img_mod = c.x_mod;
    const Act& ho = u->acts[u->head_out];
    h.stats = ho.stats != SIZE_MAX ? (float*)(u->ws + ho.stats) : nullptr;
    hipError_t e;
    if (u->head_wmf != SIZE_MAX) {
      h.wmf = (const bf16_t*)(u->wdev + u->head_wmf);
      e = launch_head_mfma(h, s);
    } else {
      e = u->bf16 ? launch_head<bf16_t>(h, s) : launch_head<float>(h, s);
    }
    return e == hipSuccess ? ITSD_OK : fail(ITSD_ERR_HIP, hipGetErrorString(e));
  }));
  // census kinds: OpKind, and kCensusConvGN for the fused GroupNorm+SiLU convs
  for (size_t oi = 0; oi < u->ops.size(); ++oi) {
    const Op& o = u->ops[oi];
    if (folded_into(u, rp, oi) >= 0) continue;
    const ConvLaunch& cl = rp[oi];
    int kind = o.kind == OP_ATTNBLOCK ? kCensusAttnBlock : (int)o.kind;
    cur_op = (int)oi + 1;
    if (o.kind == OP_CONV && o.coef != SIZE_MAX)
      kind = cl.p.wide_segs == 1 ? kCensusConvGNW : cl.p.wide_segs == 4 ? kCensusConvGNW4 : kCensusConvGN;
    double fl = op_flops(u, o, c.nb);
    // + the folded shortcut's K slices (1x1, its Cin)
    if (cl.p.sc_split) fl += 2.0 * cl.a.M * (double)o.Cout * (cl.a.sc_C1 + cl.a.sc_C2);
    CHK(mark(kind, fl, [&]() { return launch_op(u, o, c, &cl, s); }));
  }
  // tail GN + conv (+ sampler update); bf16 MFMA tail: GN coefficients, then one fused launch
  cur_op = 0;
  Op g;
  g.src1 = u->tail_in; g.gamma = u->tail_gn_g; g.beta = u->tail_gn_b; g.silu = 1;
  if (u->tail_wmf != SIZE_MAX) {
    g.kind = OP_GNCOEF;
    g.coef = u->tail_coef;
  } else {
    g.kind = OP_GN;
    g.dst = u->tail_g;
  }
  CHK(mark((int)g.kind, 0.0, [&]() { return launch_op(u, g, c, nullptr, s); }));
  CHK(mark(-2, 2.0 * c.tail.n * (c.tail.cfg ? 2 : 1) * u->H * u->H * 27.0 * u->acts[u->tail_in].C, [&]() -> int {
    TailArgs t = c.tail;
    t.w = u->wp(u->tail_w);
    t.b = u->wp(u->tail_b);
    t.H = u->H; t.W = u->H; t.C = u->acts[u->tail_in].C;
    hipError_t e;
    if (u->tail_wmf != SIZE_MAX) {
      t.g = u->ap(u->tail_in);
      t.coef = (const float*)(u->ws + u->tail_coef);
      t.wmf = (const bf16_t*)(u->wdev + u->tail_wmf);
      e = launch_tail_mfma(t, s);
    } else {
      t.g = u->ap(u->tail_g);
      e = u->bf16 ? launch_tail<bf16_t>(t, s) : launch_tail<float>(t, s);
    }
    return e == hipSuccess ? ITSD_OK : fail(ITSD_ERR_HIP, hipGetErrorString(e));
  }));
  return ITSD_OK;
}

// temb rows: out[m][sumC] = Wp^T silu(MLP(emb(idx[m]))) + bp (Model.py:51-93 then each
// ResBlock's temb_proj, :175-178); cond=true uses the label table / cond MLP.
int temb_rows(itsd_unet* u, const int* idx, int M, int offset, bool cond, float* out, hipStream_t s) {
  if (M > u->rows_cap) return fail(ITSD_ERR_INVALID, "temb rows exceed capacity");
  const int ch = u->ch, td = u->tdim;
  hipError_t e;
  if (!cond) {
    e = launch_emb_input(idx, M, u->cfg ? nullptr : u->wp(u->freq), u->cfg ? u->wp(u->ttable) : nullptr, ch,
                         u->emb_buf, offset, s);
  } else {
    e = launch_emb_input(idx, M, nullptr, u->wp(u->ctable), ch, u->emb_buf, offset, s);
  }
  if (e != hipSuccess) return fail(ITSD_ERR_HIP, hipGetErrorString(e));
  const float* W0 = u->wp(cond ? u->C1t : u->W0t);
  const float* b0 = u->wp(cond ? u->cb1 : u->b0);
  const float* W2 = u->wp(cond ? u->C3t : u->W2t);
  const float* b2 = u->wp(cond ? u->cb3 : u->b2);
  HIPCHK(launch_linear(u->emb_buf, M, ch, W0, b0, td, 0, u->h1_buf, s));
  HIPCHK(launch_linear(u->h1_buf, M, td, W2, b2, td, 1, u->te_buf, s));
  HIPCHK(launch_linear(u->te_buf, M, td, u->wp(cond ? u->Wct : u->Wpt), u->wp(cond ? u->bc : u->bp), u->sumC, 1,
                       out, s));
  return ITSD_OK;
}

int alloc_rows(itsd_unet* u, int rows) {
  if (rows <= u->rows_cap) return ITSD_OK;
  hipFree(u->emb_buf); hipFree(u->h1_buf); hipFree(u->te_buf);
  HIPCHK(hipMalloc(&u->emb_buf, (size_t)rows * u->ch * 4));
  HIPCHK(hipMalloc(&u->h1_buf, (size_t)rows * u->tdim * 4));
  HIPCHK(hipMalloc(&u->te_buf, (size_t)rows * u->tdim * 4));
  u->rows_cap = rows;
  return ITSD_OK;
}

void clear_graphs(itsd_unet* u) {
  for (auto& g : u->graphs)
    if (g.exec) hipGraphExecDestroy(g.exec);
  u->graphs.clear();
}

// Either schedule call starts here: no step graph, no table of the previous schedule, of either form, and no attached
// trace survives (T_sched = 0 until the new one is complete, so a failed call leaves the handle without a schedule).
void drop_schedule(itsd_unet* u) {
  clear_graphs(u);
  u->trace = nullptr;
  u->trace_rows = u->trace_stride = 0;
  u->guidance = 0;  // (the device buffers stay: no graph that reads them survives clear_graphs)
  u->gw_rows_h.clear();
  u->gw_img_h.clear();
  hipFree(u->coeff1); hipFree(u->coeff2); hipFree(u->sqrt_var); hipFree(u->xrow); hipFree(u->temb_table);
  u->coeff1 = u->coeff2 = u->sqrt_var = u->xrow = u->temb_table = nullptr;
  u->T_sched = 0;
  u->sched_form = 0;
  u->clip_x0 = 0;
  u->hist_row = -1;
  u->hist_n = 0;
}

int check_batch(itsd_unet* u, int n) {
  if (n <= 0 || n > u->d.max_batch)
    return fail(ITSD_ERR_INVALID, "batch " + std::to_string(n) + " outside [1, max_batch=" +
                                      std::to_string(u->d.max_batch) + "]");
  return ITSD_OK;
}

// itsd_verify_denoise's two scratch buffers (itsd_unet::vd_xt, vd_part): the smallest tail block is 64 pixels
size_t vd_xt_bytes(const itsd_unet* u) { return (size_t)u->d.max_batch * 3 * u->H * u->H * 4; }
size_t vd_part_bytes(const itsd_unet* u) { return (size_t)u->d.max_batch * ((u->H * u->H + 63) / 64) * 2 * 4; }
size_t tr_part_bytes(const itsd_unet* u) { return 2 * vd_part_bytes(u); }  // (four floats a block)

// The two pass shapes. forward: one time-embedding row an image (proj_buf, from temb_rows), the batch as given, the
// tail writes eps to eps_out.
RunCtx forward_ctx(const itsd_unet* u, int n, const float* x, const int32_t* labels, float* eps_out) {
  RunCtx c{};
  c.nb = n; c.x = x; c.x_mod = n;
  c.temb = u->proj_buf; c.tsel = nullptr; c.temb_img_stride = u->sumC;
  c.labels = labels; c.label_mod = n; c.uncond_from = -1;
  c.tail.n = n; c.tail.cfg = 0; c.tail.step_mode = kTailEps; c.tail.eps_out = eps_out;
  return c;
}

// step: the sampler's program on the state x -- the schedule's time-embedding table, its row selected on the device
// through d_t, the doubled cond||uncond batch and the guided tail for CFG. The caller sets tail.step_mode and that
// mode's operands.
RunCtx step_ctx(const itsd_unet* u, int n, float* x, const int32_t* labels) {
  RunCtx c{};
  c.nb = u->cfg ? 2 * n : n;
  c.x = x; c.x_mod = n;
  c.temb = u->temb_table; c.tsel = u->d_t; c.temb_img_stride = 0;
  c.labels = labels; c.label_mod = n; c.uncond_from = u->cfg ? n : -1;
  c.tail.n = n; c.tail.cfg = u->cfg ? 1 : 0; c.tail.guide_w = u->guide_w; c.tail.guide_w1 = u->guide_w1;
  c.tail.x = x;
  return c;
}

// The stream hand-over of an entry point that works on u->stream for a caller on another stream. enter: the handle's
// device is made current and u->stream waits for what the caller's stream (cs) has queued; leave (the success path
// only): the caller's stream waits for what u->stream has queued.
int enter_stream(itsd_unet* u, hipStream_t cs) {
  HIPCHK(hipSetDevice(u->device));
  HIPCHK(hipEventRecord(u->ev_in, cs));
  HIPCHK(hipStreamWaitEvent(u->stream, u->ev_in, 0));
  return ITSD_OK;
}
int leave_stream(itsd_unet* u, hipStream_t cs) {
  HIPCHK(hipEventRecord(u->ev_out, u->stream));
  HIPCHK(hipStreamWaitEvent(cs, u->ev_out, 0));
  return ITSD_OK;
}

// The step graph of (n, labels present, noise pointer, option generation, schedule form, trace pointer and stride,
// guidance table kind, cond-only program; keep: an entry the eviction passes over, the run's other graph):
// the cached one, or one step of c (the program -- the trace's finalize launch rides behind the tail -- then the step
// counter's decrement) captured on u->stream, instantiated and cached -- 4 entries, the oldest out. The trace is in the
// key because its pointer is baked into the captured launches: a graph captured untraced is never replayed traced. A
// failed capture is ended and its graph destroyed before the error is returned.
int step_graph(itsd_unet* u, const RunCtx& c, int n, bool labels, const float* noise, hipGraphExec_t* exec,
               bool cond_only = false, hipGraphExec_t keep = nullptr) {
  const auto key = std::make_tuple(n, labels, noise, itsd::g_option_gen, u->sched_form, (const double*)u->trace,
                                   u->trace_stride, u->guidance, cond_only);
  for (auto& g : u->graphs)
    if (g.key == key) { *exec = g.exec; return ITSD_OK; }
  hipStream_t s = u->stream;
  HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  int r = run_program(u, c, resolve_program(u, c), s);
  if (r == ITSD_OK && launch_add_int(u->d_t, -1, s) != hipSuccess) r = fail(ITSD_ERR_HIP, "add_int");
  hipGraph_t graph = nullptr;
  hipError_t e = hipStreamEndCapture(s, &graph);
  if (r != ITSD_OK) { if (graph) hipGraphDestroy(graph); return r; }
  if (e != hipSuccess) return fail(ITSD_ERR_HIP, std::string("capture: ") + hipGetErrorString(e));
  e = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
  hipGraphDestroy(graph);
  if (e != hipSuccess) return fail(ITSD_ERR_HIP, std::string("instantiate: ") + hipGetErrorString(e));
  if (u->graphs.size() >= 4) {  // the oldest out, but never the graph this run is about to launch as well
    auto old = u->graphs.begin();
    if (keep && old->exec == keep) ++old;
    hipGraphExecDestroy(old->exec);
    u->graphs.erase(old);
  }
  u->graphs.push_back({key, *exec});
  ++u->graph_captures;
  return ITSD_OK;
}

// What a profile entry point holds for one call: the eps output, CFG's all-zero labels (the unconditional row for
// every image: the guided batch's launches, shapes and FLOPs), the event pairs and the census's per-launch records.
// The destructor releases them on every return path, a failed run's events included.
struct ProfileScratch {
  float* eps = nullptr;
  int32_t* lab0 = nullptr;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> evs;
  std::vector<int> kinds, kid, eop;
  std::vector<double> fl;
  ~ProfileScratch() {
    for (auto& p : evs) {
      if (p.first) hipEventDestroy(p.first);
      if (p.second) hipEventDestroy(p.second);
    }
    hipFree(eps);
    hipFree(lab0);
  }
  // What the three entry points open with: the caller's stream (cs) drained, the buffers, one time-embedding row an
  // image in proj_buf.
  int begin(itsd_unet* u, const int32_t* t, int n, hipStream_t cs) {
    CHK(check_batch(u, n));
    HIPCHK(hipSetDevice(u->device));
    u->last_forward_n = 0;  // (the tail input is overwritten: itsd_unet_representation refuses until the next forward)
    HIPCHK(hipStreamSynchronize(cs));
    HIPCHK(hipMalloc(&eps, (size_t)n * 3 * u->H * u->H * 4));
    if (u->cfg) {
      HIPCHK(hipMalloc(&lab0, (size_t)n * 4));
      HIPCHK(hipMemsetAsync(lab0, 0, (size_t)n * 4, u->stream));
    }
    return temb_rows(u, t, n, 0, false, u->proj_buf, u->stream);
  }
  // c records its launches here (ids: also each launch's kernel id and program op)
  void census(RunCtx& c, bool ids) {
    c.census = true; c.evs = &evs; c.ev_kind = &kinds; c.ev_flops = &fl;
    if (ids) { c.ev_kid = &kid; c.ev_op = &eop; }
  }
};

}  // namespace

// ============================================================================ C ABI
namespace itsd {
thread_local const char* g_last_kernel = nullptr;
std::mutex& kernel_names_mu() {
  static std::mutex m;
  return m;
}
std::vector<const char*>& kernel_names() {
  static std::vector<const char*> v;
  return v;
}
// ids of launch-site names: 0 = none recorded, else 1 + index in kernel_names() (the names are
// the ITSD_LAUNCH string literals, so equal sites compare equal by content)
int kernel_id(const char* name) {
  if (!name) return 0;
  std::lock_guard<std::mutex> lk(kernel_names_mu());
  auto& v = kernel_names();
  for (size_t i = 0; i < v.size(); ++i)
    if (v[i] == name || !std::strcmp(v[i], name)) return (int)i + 1;
  v.push_back(name);
  return (int)v.size();
}
}  // namespace itsd

namespace {
// itsd_set_option's keys (include/itsd.h lists the same set). A value outside [lo, hi] is refused, except:
enum : unsigned {
  kDiag = 1,   // a measured-and-dropped variant's switch (round 6): diagnostic builds only
               // (tools/build_diag.sh); the shipped library refuses the key
  kShip1 = 2,  // the shipped library takes [lo, 1] only (above: a diagnostic variant)
  kBool = 4,   // any value, stored as 0 / 1
  kSet = 8,    // the values listed in `set` (ended by -1)
  kMask = 16,  // any value, stored & hi
};
struct Option {
  const char* key;
  int* var;
  int lo, hi;
  unsigned flags;
  const char* what;
  int set[6] = {-1, -1, -1, -1, -1, -1};
};
// conv_dbg (measurements only: results are wrong when set): 1 no in-loop loads (zero-page sources), 2 no MFMA, 8 no GN
// transform, 16 no epilogue, 32 no epilogue output stores, 64 fused-conv halo loads from the zero page, 128 no GN
// statistics pass, 256 no residual loads, 512 (wide fused conv) s_setprio 1 for waves 4-7 (results unchanged),
// 1024 / 2048 (wide fused conv) every lane reads the same B / A fragment row (LDS broadcast). (Never skip an issued
// load's wait: an in-flight load landing in a reused register faults.) 4096 | (mask << 13): compile-time ablations of
// conv3x3_gn_p4_kernel<32> (conv.hip); (1 << 20) / (1 << 21): s_setprio 1 / 2 for the fused GroupNorm conv's halo waves
constexpr int kConvDbgMask = 1 | 2 | 8 | 16 | 32 | 64 | 128 | 256 | 512 | 1024 | 2048 | 4096 | (127 << 13) | (3 << 20);
const Option kOptions[] = {
    {"conv_variant", &g_conv_variant, 1, 2, 0, "2 conv_pipe (shipped), 1 conv_igemm (register-staged, parity checks)"},
    {"splitk", &g_splitk, 0, 64, kShip1, "split-K for under-filled grids: 0 off, 1 auto, >= 2 forced slice count"},
    {"splitk_inl", &g_splitk_inl, 0, 1, 0, "conv_pipe split-K: 1 in-launch ticket combine, 0 splitk_epilogue_kernel"},
    {"subpix_split", &g_subpix_split, 0, 1, 0, "under-filled sub-pixel conv_pipe launches split K in-launch"},
    {"conv1x1", &g_conv1x1, 0, 2, kShip1, "streaming 1x1 kernel for statistics-free 1x1 convs of large pixel counts: 0 off, 1 on, 2 the 7-stage ring"},
    {"small_conv", &g_small_conv, 0, 2, 0, "conv_small's 64x64 tiles at the small levels: 0 off, 1 auto, 2 whenever eligible"},
    {"small_8x8", &g_small_8x8, 0, 1, 0, "conv_small (split K) for under-filled 8x8-level convs"},
    {"small_wide", &g_small_wide, 0, 2, 0, "conv_small for under-filled statistics-free convs of larger images: 0 off, 1 under 256 tiles, 2 under 512"},
    {"small_minks", &g_small_minks, 1, 64, kDiag, "conv_small split K: at least this many 64-channel K-chunks a slice"},
    {"small_gn", &g_small_gn, 0, 1, 0, "conv_small writes its consumer GroupNorm's output (the GN launch skipped): 0 off, 1 on"},
    {"conv_dbg", &g_conv_dbg, 0, kConvDbgMask, kDiag | kMask, "measurement-only conv ablations (a bit mask; results are wrong when set)"},
    {"fuse_gn", &g_fuse_gn, 0, 1, kBool, "fused GroupNorm+SiLU+conv3x3 in ResBlocks (UNets created afterwards)"},
    {"gn_wide", &g_gn_wide, 0, 2, 0, "the persistent 256-pixel fused conv: 0 off, 1 auto, 2 whenever eligible"},
    {"gn_fold", &g_gn_fold, 0, 1, kBool, "GroupNorm finalize inside conv3x3_gn_p4 / p5_kernel: 0 off, 1 on"},
    {"p4_w", &g_p4_w, 0, 7, 0, "levels conv3x3_gn_p4_kernel takes (bit 0 W = 8, 1 W = 16, 2 W = 32); the others run p5 / 128-pixel tiles"},
    {"p4_xcd", &g_p4_xcd, 0, 2, kDiag, "conv3x3_gn_p4_kernel deals each XCD a contiguous range of tiles: 0 off, 1 on, 2 the 8x8 level only"},
    {"p4_c96", &g_p4_c96, 0, 2, 0, "8x8 conv3x3_gn_p4_kernel on 96-cout tiles: 0 off, 1 auto, 2 always (Cout % 96 == 0)"},
    {"p4_sub", &g_p4_sub, 0, 1, 0, "nearest-x2 upsample convs on conv3x3_gn_p4_kernel's sub-pixel form: 0 off, 1 on"},
    {"p4_plain", &g_p4_plain, 0, 2, 0, "plain 3x3 stride-1 convs on conv3x3_gn_p4_kernel (halo copies the input): 0 off, 1 from 128 tiles, 2 any tile count"},
    {"p5", &g_p5, 0, 2, 0, "conv3x3_gn_p5_kernel at 8x8: 0 off, 1 auto, 2 always (4x4: always)"},
    {"p5_split", &g_p5_split, 0, 16, 0, "p5's K slices: 0 auto (cost model), 1..16 forced"},
    {"p5_sc", &g_p5_sc, 0, 2, 0, "ResBlock 1x1 shortcuts as K slices of their block2 p5 conv: 0 off, 1 auto, 2 always"},
    {"p5_pub", &g_p5_pub, 0, 1, 0, "p5's two-slice last-arriver combine: 1 only the first arriver stores its partial, 0 both (round 5; bit-identity checks)"},
    {"p5_xl", &g_p5_xl, 0, 3, 0, "p5's split-K partials through one XCD's L2: 0 off, 1 the shared combine at 8x8 / 16x16, 2 every eligible form (A/B), 3 (shipped) 1 + the two-slice form at 8x8 / 16x16 where K <= 3456"},
    {"p5_dist", &g_p5_dist, 0, 2, 0, "p5's split-K combine shared by every slice (co-resident grids): 0 off (last arriver), 1 on, 2 the plans of 1 combined by the last arriver (bit-identity checks)"},
    {"p5_c64", &g_p5_c64, 0, 2, kDiag, "64-cout conv3x3_gn_p5_kernel items at 8x8 / 4x4: 0 off, 1 auto, 2 always"},
    {"convt_prune", &g_convt_prune, 0, 1, 0, "ConvTranspose2d sub-pixel phases skip their all-zero taps (p4 / conv_pipe)"},
    {"tap_prune", &g_tap_prune, 0, 1, kBool, "drop all-padding conv taps at build time (UNets created afterwards)"},
    {"down_merge", &g_down_merge, 0, 1, kBool, "CFG DownSample c1 + c2 as one 5x5 conv (UNets created afterwards)"},
    {"io_mfma", &g_io_mfma, 0, 1, kBool, "bf16 head / tail on MFMA (UNets created afterwards)"},
    {"attn_fuse", &g_attn_fuse, 0, 1, 0, "fused AttnBlock kernel (S = 64): 0 off, 1 on (UNets created afterwards; the 16-token form was removed)"},
    {"attn_s1", &g_attn_s1, 0, 1, 0, "one-token AttnBlock folded to GroupNorm + one 1x1 conv (UNets created afterwards)"},
    {"attn_split", &g_attn_split, 0, 6, kSet, "attn_block_split_kernel (an image over G blocks): 0 off, 1 auto, 2 / 4 / 6 forced", {0, 1, 2, 4, 6, -1}},
    {"attn_wide", &g_attn_wide, 0, 2, 0, "channel-split attention (attn_cs_kernel): 0 off, 1 auto (C >= 384 at S >= 256; C = 1024), 2 wherever it applies"},
    {"attn_wide_nq", &g_attn_wide_nq, 0, 2, 0, "channel-split attention: query groups a block (0 auto, 1, 2)"},
    {"attn_cs", &g_attn_cs, 0, 8, kDiag, "attn_mfma_kernel output-channel slices: 0 auto, 1..8 forced"},
    {"attn_aq", &g_attn_aq, 0, 64, kDiag | kSet, "attn_mfma_kernel queries per block: 0 auto, 32, 64", {0, 32, 64, -1}},
    {"cfg_skip", &g_cfg_skip, 0, 1, 0, "rows of a guidance table with w == 0 run the cond-only step program (batch n): 0 off (the doubled batch through the table), 1 on"},
    {"spin_bound", &g_spin_bound, 0, 0x7fffffff, 0, "diagnostic: polls before an in-kernel hand-off wait fails (shipped 1 << 22)"},
};
}  // namespace

extern "C" {

int itsd_version(void) { return 1; }

const char* itsd_kernel_name(int id) {
  std::lock_guard<std::mutex> lk(itsd::kernel_names_mu());
  return id > 0 && id <= (int)itsd::kernel_names().size() ? itsd::kernel_names()[id - 1] : "";
}

int itsd_set_option(const char* key, int value) {
  if (!key) return fail(ITSD_ERR_INVALID, "null key");
#ifdef ITSD_DIAG
  const bool shipped = false;
#else
  const bool shipped = true;
#endif
  const Option* o = nullptr;
  for (const Option& r : kOptions)
    if (!std::strcmp(key, r.key)) o = &r;
  if (o && shipped && (o->flags & kDiag))
    return fail(ITSD_ERR_INVALID, std::string(key) + ": diagnostic builds only (tools/build_diag.sh)");
  if (o && shipped && (o->flags & kShip1) && value > 1)
    return fail(ITSD_ERR_INVALID, std::string(key) + " in [" + std::to_string(o->lo) + ",1] (above: diagnostic builds only, tools/build_diag.sh)");
  ++itsd::g_option_gen;  // cached step graphs baked in the previous kernel choices
  if (!o) return fail(ITSD_ERR_INVALID, std::string("unknown option ") + key);
  // validated before it is stored: a refused call leaves the previous setting in place
  int v = value;
  if (o->flags & kBool) {
    v = value ? 1 : 0;
  } else if (o->flags & kMask) {
    v = value & o->hi;
  } else if (o->flags & kSet) {
    bool ok = false;
    std::string vals;
    for (const int* q = o->set; *q >= 0; ++q) {
      ok |= *q == value;
      vals += (vals.empty() ? "" : ",") + std::to_string(*q);
    }
    if (!ok) return fail(ITSD_ERR_INVALID, std::string(key) + " in {" + vals + "}: " + o->what);
  } else if (value < o->lo || value > o->hi) {
    return fail(ITSD_ERR_INVALID, std::string(key) + " in [" + std::to_string(o->lo) + "," + std::to_string(o->hi) + "]: " + o->what);
  }
  *o->var = v;
  return ITSD_OK;
}

const char* itsd_last_error(void) { return g_err.c_str(); }

int itsd_calibrate(int what, double* value, void* stream) {
  if (!value) return fail(ITSD_ERR_INVALID, "null argument");
  if (what != ITSD_CALIB_MFMA_BF16 && what != ITSD_CALIB_HBM_COPY && what != ITSD_CALIB_MFMA_BF16_16X16) return fail(ITSD_ERR_INVALID, "unknown calibration");
  const int rc = calibrate_run(what, value, (hipStream_t)stream);
  if (rc == ITSD_ERR_OOM) return fail(rc, "calibration buffers (2 x 1 GiB)");
  if (rc != ITSD_OK) return fail(rc, "calibration kernel");
  return ITSD_OK;
}

int itsd_unet_query(const itsd_unet* u, const char* key, int64_t* value) {
  if (!u || !key || !value) return fail(ITSD_ERR_INVALID, "null argument");
  if (!std::strcmp(key, "graph_captures")) *value = u->graph_captures;
  else if (!std::strcmp(key, "max_batch")) *value = u->d.max_batch;
  else if (!std::strcmp(key, "T_sched")) *value = u->T_sched;
  else if (!std::strcmp(key, "sched_form")) *value = u->sched_form;
  else if (!std::strcmp(key, "trace")) *value = u->trace ? 1 : 0;
  else if (!std::strcmp(key, "guidance")) *value = u->guidance;
  else if (!std::strcmp(key, "cond_only_steps")) *value = u->cond_only_steps;
  else if (!std::strcmp(key, "ws_bytes")) *value = (int64_t)u->ws_bytes;
  else if (!std::strcmp(key, "ops")) *value = (int64_t)u->ops.size();
  else if (!std::strcmp(key, "status")) {  // synchronous: the in-kernel hand-off status word of the last forward / run
    if (hipStreamSynchronize(u->stream) != hipSuccess) return fail(ITSD_ERR_HIP, "status: stream synchronize");
    int flag = 0;
    if (hipMemcpy(&flag, u->d_nan + 1, 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(ITSD_ERR_HIP, "status: copy");
    *value = flag;
  }
  else return fail(ITSD_ERR_INVALID, std::string("unknown query key ") + key);
  return ITSD_OK;
}

int itsd_unet_create(const itsd_unet_desc* desc, const itsd_tensor_view* weights, int n_weights, int device,
                     itsd_unet** out) {
  if (!desc || !out || (!weights && n_weights)) return fail(ITSD_ERR_INVALID, "null argument");
  const itsd_unet_desc& d = *desc;
  if (d.arch != ITSD_ARCH_DDPM && d.arch != ITSD_ARCH_CFG) return fail(ITSD_ERR_INVALID, "unknown arch");
  if (d.ch <= 0 || d.ch % 32 || d.n_mult < 1 || d.n_mult > 8 || d.n_attn < 0 || d.n_attn > 8 ||
      d.num_res_blocks < 1 || d.max_batch < 1 || d.img_size < 8)
    return fail(ITSD_ERR_INVALID, "invalid UNet descriptor");
  if (d.img_size % (1 << (d.n_mult - 1))) return fail(ITSD_ERR_INVALID, "img_size not divisible by the down path");
  for (int k = 0; k < d.n_attn; ++k)
    if (d.attn[k] < 0 || d.attn[k] >= d.n_mult) return fail(ITSD_ERR_INVALID, "attn index out of bound");
  if (d.precision != ITSD_PREC_FP32 && d.precision != ITSD_PREC_BF16) return fail(ITSD_ERR_INVALID, "precision");
  HIPCHK(hipSetDevice(device));
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
      itsd::g_num_cus = cus;
  }
  std::unique_ptr<itsd_unet> u(new itsd_unet());
  u->d = d;
  u->device = device;
  u->bf16 = d.precision == ITSD_PREC_BF16;
  u->esz = u->bf16 ? 2 : 4;
  u->cfg = d.arch == ITSD_ARCH_CFG;
  u->nb_max = d.max_batch * (u->cfg ? 2 : 1);
  CHK(build(u.get(), weights, n_weights));
  HIPCHK(hipStreamCreateWithFlags(&u->stream, hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(&u->ev_in, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&u->ev_out, hipEventDisableTiming));
  HIPCHK(hipMalloc(&u->d_t, 64));
  HIPCHK(hipMalloc(&u->d_nan, 64));
  HIPCHK(hipMalloc(&u->d_run, sizeof(RunParams)));
  HIPCHK(hipMemset(u->d_run, 0, sizeof(RunParams)));
  HIPCHK(hipMalloc(&u->x_state, (size_t)d.max_batch * 3 * d.img_size * d.img_size * 4));
  HIPCHK(hipMalloc(&u->lab_state, (size_t)d.max_batch * 4));
  HIPCHK(hipMalloc(&u->zero_page, 64 * 4096 + 1024));
  HIPCHK(hipMemset(u->zero_page, 0, 64 * 4096 + 1024));
  HIPCHK(hipMalloc(&u->splitk_ws, itsd_unet::kSplitkCap * 4));
  HIPCHK(hipMalloc(&u->tickets, itsd::kTicketCap * 4));
  HIPCHK(hipMemset(u->tickets, 0, itsd::kTicketCap * 4));
  HIPCHK(hipMalloc(&u->attn_sync, (size_t)u->nb_max * 4));
  HIPCHK(hipMemset(u->attn_sync, 0, (size_t)u->nb_max * 4));
  HIPCHK(hipMalloc(&u->proj_buf, (size_t)d.max_batch * u->sumC * 4));
  CHK(alloc_rows(u.get(), std::max(d.max_batch, d.num_labels + 1)));
  if (u->cfg) {
    HIPCHK(hipMalloc(&u->cemb_table, (size_t)(d.num_labels + 1) * u->sumC * 4));
    CHK(temb_rows(u.get(), nullptr, d.num_labels + 1, 0, true, u->cemb_table, u->stream));
    HIPCHK(hipStreamSynchronize(u->stream));
  }
  *out = u.release();
  return ITSD_OK;
}

int itsd_unet_destroy(itsd_unet* u) {
  if (!u) return ITSD_OK;
  hipSetDevice(u->device);
  clear_graphs(u);
  hipFree(u->wdev); hipFree(u->ws); hipFree(u->emb_buf); hipFree(u->h1_buf); hipFree(u->te_buf);
  hipFree(u->proj_buf); hipFree(u->cemb_table); hipFree(u->coeff1); hipFree(u->coeff2); hipFree(u->sqrt_var);
  hipFree(u->xrow); hipFree(u->temb_table); hipFree(u->d_t); hipFree(u->d_nan); hipFree(u->d_run); hipFree(u->x0_hist); hipFree(u->x_state); hipFree(u->lab_state); hipFree(u->zero_page);
  hipFree(u->splitk_ws);
  hipFree(u->tickets);
  hipFree(u->attn_sync);
  hipFree(u->vd_xt);
  hipFree(u->vd_part);
  hipFree(u->tr_part);
  hipFree(u->gw_rows_d);
  hipFree(u->gw_img_d);
  if (u->stream) hipStreamDestroy(u->stream);
  if (u->ev_in) hipEventDestroy(u->ev_in);
  if (u->ev_out) hipEventDestroy(u->ev_out);
  delete u;
  return ITSD_OK;
}

int itsd_unet_forward(itsd_unet* u, const float* x, const int32_t* t, const int32_t* labels, float* eps, int n,
                      void* stream) {
  if (!u || !x || !t || !eps) return fail(ITSD_ERR_INVALID, "null argument");
  if (u->cfg && !labels) return fail(ITSD_ERR_INVALID, "CFG UNet needs labels");
  CHK(check_batch(u, n));
  hipStream_t cs = (hipStream_t)stream;
  hipStream_t s = u->stream;
  CHK(enter_stream(u, cs));
  CHK(temb_rows(u, t, n, 0, false, u->proj_buf, s));
  const RunCtx c = forward_ctx(u, n, x, labels, eps);
  HIPCHK(hipMemsetAsync(u->d_nan + 1, 0, 4, s));  // this forward's hand-off status (itsd_unet_query "status")
  CHK(run_program(u, c, resolve_program(u, c), s));
  u->last_forward_n = n;
  return leave_stream(u, cs);
}

int itsd_unet_representation(itsd_unet* u, float* repr, int n, void* stream) {
  if (!u || !repr) return fail(ITSD_ERR_INVALID, "null argument");
  if (u->last_forward_n == 0) return fail(ITSD_ERR_INVALID, "itsd_unet_representation: no itsd_unet_forward on this handle yet");
  if (n < 1 || n > u->last_forward_n)
    return fail(ITSD_ERR_INVALID, "itsd_unet_representation: n outside [1, last forward's batch]");
  const Act& A = u->acts[u->tail_in];
  hipStream_t cs = (hipStream_t)stream;
  hipStream_t s = u->stream;
  CHK(enter_stream(u, cs));
  HIPCHK(u->bf16 ? launch_nhwc_to_nchw<bf16_t>(u->ap(u->tail_in), repr, n, A.H * A.W, A.C, s)
                 : launch_nhwc_to_nchw<float>(u->ap(u->tail_in), repr, n, A.H * A.W, A.C, s));
  return leave_stream(u, cs);
}

int itsd_set_schedule(itsd_unet* u, int T, const float* coeff1, const float* coeff2, const float* sqrt_var, float w) {
  if (!u || T < 1 || !coeff1 || !coeff2 || !sqrt_var) return fail(ITSD_ERR_INVALID, "bad schedule");
  if (u->cfg && T > u->d.T)
    return fail(ITSD_ERR_INVALID, "CFG time-embedding table has " + std::to_string(u->d.T) + " rows < sampler T");
  HIPCHK(hipSetDevice(u->device));
  drop_schedule(u);
  HIPCHK(hipMalloc(&u->coeff1, T * 4));
  HIPCHK(hipMalloc(&u->coeff2, T * 4));
  HIPCHK(hipMalloc(&u->sqrt_var, T * 4));
  HIPCHK(hipMemcpy(u->coeff1, coeff1, T * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(u->coeff2, coeff2, T * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(u->sqrt_var, sqrt_var, T * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMalloc(&u->temb_table, (size_t)T * u->sumC * 4));
  CHK(alloc_rows(u, T));
  CHK(temb_rows(u, nullptr, T, 0, false, u->temb_table, u->stream));
  HIPCHK(hipStreamSynchronize(u->stream));
  u->T_sched = T;
  u->guide_w = w;
  u->guide_w1 = (float)(1.0 + (double)w);
  return ITSD_OK;
}

// The x0-form schedules: K rows, row k run at timestep tau[k]. The time-embedding table is built for tau (temb_rows with
// a device copy of it), so everything downstream -- the step program, itsd_sampler_predict_x0 -- indexes by row.
// cp: null for itsd_set_schedule_x0 (form 1); the sixth table of itsd_set_schedule_x0_2m (form 2), which also owns the
// x0 history. fn names the entry point in every refusal; all of them come before the first HIP call.
static int install_x0_schedule(itsd_unet* u, const itsd_x0_schedule* sc, const float* cp, bool two_m, const char* fn) {
  const std::string who = std::string(fn) + ": ";
  if (!sc) return fail(ITSD_ERR_INVALID, who + "null schedule");
  if (!sc->tau || !sc->a0 || !sc->b0 || !sc->c0 || !sc->cx || !sc->sg || (two_m && !cp))
    return fail(ITSD_ERR_INVALID, who + "null table");
  const int K = sc->K;
  if (K < 1) return fail(ITSD_ERR_INVALID, who + "K = " + std::to_string(K) + " < 1");
  for (int k = 0; k < K; ++k)
    if (sc->tau[k] < 0 || (k && sc->tau[k] <= sc->tau[k - 1]))
      return fail(ITSD_ERR_INVALID, who + "tau[" + std::to_string(k) + "] = " + std::to_string(sc->tau[k]) +
                                        ": timesteps must be >= 0 and strictly increasing");
  if (sc->clip_x0 != 0 && sc->clip_x0 != 1)
    return fail(ITSD_ERR_INVALID, who + "clip_x0 = " + std::to_string(sc->clip_x0) + " is neither 0 nor 1");
  if (two_m) {
    for (int k = 0; k < K; ++k)
      if (!std::isfinite(cp[k]))
        return fail(ITSD_ERR_INVALID, who + "cp[" + std::to_string(k) + "] is not finite");
    if (cp[K - 1] != 0.f)
      return fail(ITSD_ERR_INVALID, who + "cp[K - 1] = " + std::to_string(cp[K - 1]) +
                                        " != 0: the top row has no predecessor");
  }
  if (!u) return fail(ITSD_ERR_INVALID, who + "null handle");
  if (u->cfg && sc->tau[K - 1] >= u->d.T)
    return fail(ITSD_ERR_INVALID, "CFG time-embedding table has " + std::to_string(u->d.T) + " rows <= timestep " +
                                      std::to_string(sc->tau[K - 1]));
  HIPCHK(hipSetDevice(u->device));
  drop_schedule(u);
  const int ntab = two_m ? 6 : 5;
  HIPCHK(hipMalloc(&u->xrow, (size_t)ntab * K * 4));
  const float* rows[6] = {sc->a0, sc->b0, sc->c0, sc->cx, sc->sg, cp};
  for (int i = 0; i < ntab; ++i)
    HIPCHK(hipMemcpy(u->xrow + (size_t)i * K, rows[i], (size_t)K * 4, hipMemcpyHostToDevice));
  if (two_m && !u->x0_hist) HIPCHK(hipMalloc(&u->x0_hist, vd_xt_bytes(u)));
  HIPCHK(hipMalloc(&u->temb_table, (size_t)K * u->sumC * 4));
  CHK(alloc_rows(u, K));
  int* d_tau = nullptr;
  HIPCHK(hipMalloc(&d_tau, (size_t)K * 4));
  int rc = ITSD_OK;
  if (hipMemcpy(d_tau, sc->tau, (size_t)K * 4, hipMemcpyHostToDevice) != hipSuccess) rc = fail(ITSD_ERR_HIP, "tau upload");
  if (rc == ITSD_OK) rc = temb_rows(u, d_tau, K, 0, false, u->temb_table, u->stream);
  if (rc == ITSD_OK && hipStreamSynchronize(u->stream) != hipSuccess) rc = fail(ITSD_ERR_HIP, "temb rows");
  hipFree(d_tau);
  if (rc != ITSD_OK) return rc;
  u->T_sched = K;
  u->sched_form = two_m ? 2 : 1;
  u->clip_x0 = sc->clip_x0;
  u->guide_w = sc->w;
  u->guide_w1 = (float)(1.0 + (double)sc->w);
  return ITSD_OK;
}

int itsd_set_schedule_x0(itsd_unet* u, const itsd_x0_schedule* sc) {
  return install_x0_schedule(u, sc, nullptr, false, "itsd_set_schedule_x0");
}

int itsd_set_schedule_x0_2m(itsd_unet* u, const itsd_x0_schedule* sc, const float* cp) {
  return install_x0_schedule(u, sc, cp, true, "itsd_set_schedule_x0_2m");
}

// The guidance table of the installed x0-form schedule: one weight a row, one multiplier a candidate image. Every
// refusal comes before the first HIP call. The values go to handle-owned device buffers that keep their addresses
// (the captured step graphs read them), behind whatever u->stream has queued -- a run already queued keeps the values
// it was queued under -- and the call returns once they are there, so the host copies and the device's agree.
int itsd_set_guidance(itsd_unet* u, const float* w_rows, int rows, const float* w_img, int n_img) {
  const std::string who = "itsd_set_guidance: ";
  if (!u) return fail(ITSD_ERR_INVALID, who + "null handle");
  if (!u->cfg) return fail(ITSD_ERR_INVALID, who + "not a CFG UNet (nothing to guide)");
  if (!u->T_sched || !u->sched_form)
    return fail(ITSD_ERR_INVALID, who + "no x0-form schedule installed (itsd_set_schedule_x0 / _2m; the ancestral form "
                                        "keeps its scalar w: ddim with steps = T, eta = 1 is its x0-form equivalent)");
  if (!w_rows && !w_img) {  // detach: the graphs captured without a table are still cached under their own key
    u->guidance = 0;
    u->gw_rows_h.clear();
    u->gw_img_h.clear();
    return ITSD_OK;
  }
  if (w_rows && rows != u->T_sched)
    return fail(ITSD_ERR_INVALID, who + "rows = " + std::to_string(rows) + " != T_sched = " + std::to_string(u->T_sched));
  if (w_img && (n_img < 1 || n_img > u->d.max_batch))
    return fail(ITSD_ERR_INVALID, who + "n_img = " + std::to_string(n_img) + " outside [1, max_batch=" +
                                      std::to_string(u->d.max_batch) + "]");
  for (int k = 0; w_rows && k < rows; ++k)
    if (!std::isfinite(w_rows[k])) return fail(ITSD_ERR_INVALID, who + "w_rows[" + std::to_string(k) + "] is not finite");
  for (int i = 0; w_img && i < n_img; ++i)
    if (!std::isfinite(w_img[i])) return fail(ITSD_ERR_INVALID, who + "w_img[" + std::to_string(i) + "] is not finite");
  if (tail_block_straddles(u->H, u->H, u->acts[u->tail_in].C) && u->tail_wmf == SIZE_MAX)
    return fail(ITSD_ERR_INVALID, who + "no guidance table at this tail geometry (a 256-pixel block of the generic tail "
                                        "kernel would straddle two images: H W % 256 != 0)");
  const int K = u->T_sched;
  std::vector<float> r(K, u->guide_w), m;
  if (w_rows) r.assign(w_rows, w_rows + K);
  if (w_img) m.assign(w_img, w_img + n_img);
  HIPCHK(hipSetDevice(u->device));
  if (K > u->gw_rows_cap) {  // (a larger schedule came with drop_schedule: no graph holds the old address)
    hipFree(u->gw_rows_d);
    u->gw_rows_d = nullptr;
    u->gw_rows_cap = 0;
    HIPCHK(hipMalloc(&u->gw_rows_d, (size_t)K * 4));
    u->gw_rows_cap = K;
  }
  if (!u->gw_img_d) HIPCHK(hipMalloc(&u->gw_img_d, (size_t)u->d.max_batch * 4));
  u->guidance = 0;  // (until both uploads are in place)
  HIPCHK(hipMemcpyAsync(u->gw_rows_d, r.data(), (size_t)K * 4, hipMemcpyHostToDevice, u->stream));
  if (!m.empty())
    HIPCHK(hipMemcpyAsync(u->gw_img_d, m.data(), m.size() * 4, hipMemcpyHostToDevice, u->stream));
  HIPCHK(hipStreamSynchronize(u->stream));
  u->gw_rows_h.swap(r);
  u->gw_img_h.swap(m);
  u->guidance = u->gw_img_h.empty() ? 1 : 2;
  return ITSD_OK;
}

int itsd_sampler_run(itsd_unet* u, float* x, const int32_t* labels, int n, int t_begin, int t_end, uint64_t seed,
                     int64_t noise_offset, const float* noise, uint32_t flags, void* stream) {
  if (!u || !x) return fail(ITSD_ERR_INVALID, "null argument");
  if (!u->T_sched) return fail(ITSD_ERR_INVALID, "itsd_set_schedule not called");
  if (u->cfg && !labels) return fail(ITSD_ERR_INVALID, "CFG sampler needs labels");
  CHK(check_batch(u, n));
  if (t_begin >= u->T_sched || t_end < 0 || t_end > t_begin) return fail(ITSD_ERR_INVALID, "bad step range");
  if (flags & ITSD_RUN_CONTINUE) {  // (host state only: refused before anything is queued)
    if (u->sched_form != 2)
      return fail(ITSD_ERR_INVALID, "itsd_sampler_run: ITSD_RUN_CONTINUE needs a 2M schedule (itsd_set_schedule_x0_2m): "
                                    "the other forms keep no x0 history");
    if (t_begin == u->T_sched - 1)
      return fail(ITSD_ERR_INVALID, "itsd_sampler_run: ITSD_RUN_CONTINUE at the top row " + std::to_string(t_begin) +
                                        ", which has no predecessor");
    if (u->hist_row != t_begin + 1)
      return fail(ITSD_ERR_INVALID, "itsd_sampler_run: ITSD_RUN_CONTINUE at row " + std::to_string(t_begin) +
                                        " needs the x0 of row " + std::to_string(t_begin + 1) + "; the history holds " +
                                        (u->hist_row < 0 ? std::string("none") : "row " + std::to_string(u->hist_row)));
    if (u->hist_n != n)
      return fail(ITSD_ERR_INVALID, "itsd_sampler_run: ITSD_RUN_CONTINUE with n = " + std::to_string(n) +
                                        ", the history holds " + std::to_string(u->hist_n) + " images");
  }
  if (u->trace) {  // (attached under this x0-form schedule: itsd_sampler_set_trace, drop_schedule)
    if (n > u->trace_stride)
      return fail(ITSD_ERR_INVALID, "itsd_sampler_run: batch " + std::to_string(n) + " > the attached trace's stride " +
                                        std::to_string(u->trace_stride));
    if (u->tail_wmf == SIZE_MAX && tail_block_straddles(u->H, u->H, u->acts[u->tail_in].C))
      return fail(ITSD_ERR_INVALID, "itsd_sampler_run: no score trace at this tail geometry (a 256-pixel block of the "
                                    "generic tail kernel would straddle two images: H W % 256 != 0)");
  }
  if (u->guidance == 2 && n > (int)u->gw_img_h.size())  // (attached under this x0-form schedule: itsd_set_guidance)
    return fail(ITSD_ERR_INVALID, "itsd_sampler_run: batch " + std::to_string(n) + " > the " +
                                      std::to_string(u->gw_img_h.size()) + " per-image guidance multipliers installed "
                                      "(itsd_set_guidance)");
  hipStream_t cs = (hipStream_t)stream;
  hipStream_t s = u->stream;
  CHK(enter_stream(u, cs));
  u->last_forward_n = 0;  // (the tail input is overwritten: itsd_unet_representation refuses until the next forward)
  u->cond_only_steps = 0;
  const int clip_at = (flags & ITSD_RUN_CLIP) ? t_end : -1;
  const size_t xbytes = (size_t)n * 3 * u->H * u->H * 4;
  HIPCHK(hipMemcpyAsync(u->x_state, x, xbytes, hipMemcpyDeviceToDevice, s));
  if (labels) HIPCHK(hipMemcpyAsync(u->lab_state, labels, (size_t)n * 4, hipMemcpyDeviceToDevice, s));

  RunCtx c = step_ctx(u, n, u->x_state, labels ? u->lab_state : nullptr);
  TailArgs& t = c.tail;
  const bool two_m = u->sched_form == 2;
  t.step_mode = two_m ? kTailX0Step2M : u->sched_form ? kTailX0Step : kTailStep; t.tsel = u->d_t;
  t.coeff1 = u->coeff1; t.coeff2 = u->coeff2; t.sqrt_var = u->sqrt_var;
  if (u->sched_form) {  // rows, not timesteps: d_t, the Philox stream id and the injected-noise index are the row
    for (int i = 0; i < 5; ++i) t.xrow[i] = u->xrow + (size_t)i * u->T_sched;
    t.clip_x0 = u->clip_x0;
    if (two_m) {  // (in the storage of the two ancestral pointers, null under this form)
      t.xcp = u->xrow + (size_t)5 * u->T_sched;
      t.hist = u->x0_hist;
      u->hist_row = -1;  // (until the run is queued whole)
    }
    if (u->trace) {
      t.step_mode = two_m ? kTailX0Step2MMom : kTailX0StepMom;
      t.tpart = u->tr_part; t.trace = u->trace; t.trace_rows = u->trace_rows; t.trace_stride = u->trace_stride;
    }
  }
  t.noise = noise; t.run = u->d_run; t.nan_flag = u->d_nan;
  // Under a guidance table the guided program reads its weights from the device tables (the x0-form modes' second
  // instantiations), and a row whose weight is 0 -- eps = eps_c exactly -- runs a second program, co: the n conditional
  // images with their labels through the same step mode's unguided instantiation, as the forward program runs a CFG
  // net. The host picks the program per row from its copy of the rows.
  const auto cond_only = [&](int row) { return u->guidance && g_cfg_skip && u->gw_rows_h[row] == 0.0f; };
  bool any_co = false, any_guided = false;
  for (int row = t_end; row <= t_begin; ++row) (cond_only(row) ? any_co : any_guided) = true;
  RunCtx co = c;
  if (u->guidance) {
    t.cfg = 2;
    t.gw_rows = u->gw_rows_d;  // (in the storage of the ancestral sqrt_var, null under this form)
    t.gw_img = u->guidance == 2 ? u->gw_img_d : nullptr;
    co.nb = n; co.uncond_from = -1; co.tail.cfg = 0;
  }

  RunParams rp{};
  rp.seed = seed; rp.noise_offset = noise_offset; rp.clip_at = clip_at;
  // a device parameter, so one captured step graph serves restarted and continued runs (read by the 2M modes only)
  rp.restart_at = (flags & ITSD_RUN_CONTINUE) ? -1 : t_begin;
  HIPCHK(launch_run_begin(u->d_t, t_begin, u->d_nan, u->d_run, rp, s));
  const int steps = t_begin - t_end + 1;
  if (flags & ITSD_RUN_GRAPH) {
    hipGraphExec_t exec = nullptr, exec_co = nullptr;  // (both looked up before either is launched)
    if (any_guided) CHK(step_graph(u, c, n, labels != nullptr, noise, &exec));
    if (any_co) CHK(step_graph(u, co, n, labels != nullptr, noise, &exec_co, true, exec));
    for (int i = 0; i < steps; ++i) HIPCHK(hipGraphLaunch(cond_only(t_begin - i) ? exec_co : exec, s));
  } else {
    // (the steps of one program differ in device state only)
    const std::vector<ConvLaunch> convs = any_guided ? resolve_program(u, c) : std::vector<ConvLaunch>();
    const std::vector<ConvLaunch> convs_co = any_co ? resolve_program(u, co) : std::vector<ConvLaunch>();
    for (int i = 0; i < steps; ++i) {
      const bool skip = cond_only(t_begin - i);
      CHK(run_program(u, skip ? co : c, skip ? convs_co : convs, s));
      HIPCHK(launch_add_int(u->d_t, -1, s));
    }
  }
  for (int row = t_end; row <= t_begin; ++row) u->cond_only_steps += cond_only(row) ? 1 : 0;
  HIPCHK(hipMemcpyAsync(x, u->x_state, xbytes, hipMemcpyDeviceToDevice, s));
  CHK(leave_stream(u, cs));
  if (two_m) {  // what this run leaves, for a later ITSD_RUN_CONTINUE
    u->hist_row = t_end;
    u->hist_n = n;
  }
  if (flags & ITSD_RUN_SYNC) {
    HIPCHK(hipStreamSynchronize(s));
    int flag[2] = {0, 0};
    HIPCHK(hipMemcpy(flag, u->d_nan, 8, hipMemcpyDeviceToHost));
    if (flag[1]) return fail(ITSD_ERR_HANDOFF, handoff_msg(flag[1]));
    if (flag[0]) return fail(ITSD_ERR_NAN, "nan in tensor.");
  }
  return ITSD_OK;
}

int itsd_sampler_set_trace(itsd_unet* u, double* trace, int rows, int stride) {
  if (!u) return fail(ITSD_ERR_INVALID, "itsd_sampler_set_trace: null handle");
  if (!trace) {  // detach: the graphs captured untraced are still cached under their own key
    u->trace = nullptr;
    u->trace_rows = u->trace_stride = 0;
    return ITSD_OK;
  }
  if (!u->T_sched || !u->sched_form)
    return fail(ITSD_ERR_INVALID, "itsd_sampler_set_trace: no x0-form schedule installed (itsd_set_schedule_x0 / _2m; the "
                                  "ancestral form has no x0 rows)");
  if (rows != u->T_sched)
    return fail(ITSD_ERR_INVALID, "itsd_sampler_set_trace: rows = " + std::to_string(rows) + " != T_sched = " +
                                      std::to_string(u->T_sched));
  if (stride < 1) return fail(ITSD_ERR_INVALID, "itsd_sampler_set_trace: stride = " + std::to_string(stride) + " < 1");
  if ((uintptr_t)trace % 32) return fail(ITSD_ERR_INVALID, "itsd_sampler_set_trace: trace is not 32-byte aligned");
  if (!u->tr_part) {
    HIPCHK(hipSetDevice(u->device));
    HIPCHK(hipMalloc(&u->tr_part, tr_part_bytes(u)));
  }
  u->trace = trace;
  u->trace_rows = rows;
  u->trace_stride = stride;
  return ITSD_OK;
}

// The x_0 estimate of the state x at step t: the sampler step's own program (the doubled cond||uncond batch for CFG,
// the time-embedding row selected on the device through d_t) with the tail's x0 epilogue (TailArgs::step_mode kTailX0).
// Eager, on x itself: no step graph is captured, looked up or evicted, and the sampler's run parameters and NaN flag
// stay as the last run left them.
int itsd_sampler_predict_x0(itsd_unet* u, const float* x, const int32_t* labels, int n, int t, float a0, float b0,
                            float* x0, void* stream) {
  if (!u || !x || !x0) return fail(ITSD_ERR_INVALID, "null argument");
  if (!u->T_sched) return fail(ITSD_ERR_INVALID, "itsd_set_schedule not called");
  if (u->cfg && !labels) return fail(ITSD_ERR_INVALID, "CFG sampler needs labels");
  CHK(check_batch(u, n));
  if (t < 0 || t >= u->T_sched)
    return fail(ITSD_ERR_INVALID, "step " + std::to_string(t) + " outside [0, T_sched=" + std::to_string(u->T_sched) + ")");
  if (u->guidance == 2)
    return fail(ITSD_ERR_INVALID, "itsd_sampler_predict_x0: per-image guidance multipliers are installed "
                                  "(itsd_set_guidance); the x0 epilogue guides with one scalar");
  hipStream_t cs = (hipStream_t)stream;
  hipStream_t s = u->stream;
  CHK(enter_stream(u, cs));
  u->last_forward_n = 0;  // (the tail input is overwritten: itsd_unet_representation refuses until the next forward)
  RunCtx c = step_ctx(u, n, const_cast<float*>(x), labels);
  if (u->guidance) {  // the row's weight as the scalar (host side only: kTailX0 is what it was)
    c.tail.guide_w = u->gw_rows_h[t];
    c.tail.guide_w1 = (float)(1.0 + (double)u->gw_rows_h[t]);
  }
  c.tail.step_mode = kTailX0; c.tail.a0 = a0; c.tail.b0 = b0; c.tail.x0_out = x0;
  HIPCHK(launch_set_int(u->d_t, t, s));
  HIPCHK(hipMemsetAsync(u->d_nan + 1, 0, 4, s));  // this forward's hand-off status (itsd_unet_query "status")
  CHK(run_program(u, c, resolve_program(u, c), s));
  return leave_stream(u, cs);
}

// One denoising-error probe: x0 noised to row t with the probe's own noise field (probe_noise_kernel, into the handle's
// scratch), then the sampler step's program on it -- as itsd_sampler_predict_x0: the doubled cond||uncond batch for
// CFG, the time-embedding row selected on the device -- with the tail's sse epilogue (TailArgs::step_mode kTailSse), which
// re-draws the same field and leaves sse[n][2]. Eager: no step graph is captured, looked up or evicted, and the
// sampler's run parameters and NaN flag stay as the last run left them.
int itsd_verify_denoise(itsd_unet* u, const float* x0, const int32_t* labels, int n, int t, float a, float b,
                        uint64_t seed, uint32_t stream_id, const float* noise, double* sse, float* xt_out,
                        float* eps_out, void* stream) {
  if (!u || !x0 || !sse) return fail(ITSD_ERR_INVALID, "itsd_verify_denoise: null argument");
  if (!u->T_sched) return fail(ITSD_ERR_INVALID, "itsd_verify_denoise: no schedule installed (itsd_set_schedule / _x0)");
  if (u->cfg && !labels) return fail(ITSD_ERR_INVALID, "itsd_verify_denoise: a CFG UNet needs labels");
  CHK(check_batch(u, n));
  if (t < 0 || t >= u->T_sched)
    return fail(ITSD_ERR_INVALID, "itsd_verify_denoise: step " + std::to_string(t) + " outside [0, T_sched=" +
                                      std::to_string(u->T_sched) + ")");
  hipStream_t cs = (hipStream_t)stream;
  hipStream_t s = u->stream;
  CHK(enter_stream(u, cs));
  if (!u->vd_xt) HIPCHK(hipMalloc(&u->vd_xt, vd_xt_bytes(u)));
  if (!u->vd_part) HIPCHK(hipMalloc(&u->vd_part, vd_part_bytes(u)));
  u->last_forward_n = 0;  // (the tail input is overwritten: itsd_unet_representation refuses until the next forward)
  const long long per = 3ll * u->H * u->H;
  HIPCHK(launch_probe_noise(u->vd_xt, x0, noise, n, per, a, b, seed, stream_id, s));
  if (xt_out) HIPCHK(hipMemcpyAsync(xt_out, u->vd_xt, (size_t)n * per * 4, hipMemcpyDeviceToDevice, s));
  RunCtx c = step_ctx(u, n, u->vd_xt, labels);
  TailArgs& ta = c.tail;
  ta.step_mode = kTailSse; ta.noise = noise; ta.vseed = seed; ta.vstream = stream_id;
  ta.vpart = u->vd_part; ta.vsse = sse; ta.eps_out = eps_out;
  HIPCHK(launch_set_int(u->d_t, t, s));
  HIPCHK(hipMemsetAsync(u->d_nan + 1, 0, 4, s));  // this forward's hand-off status (itsd_unet_query "status")
  CHK(run_program(u, c, resolve_program(u, c), s));
  return leave_stream(u, cs);
}

int itsd_branch(float* dst, const float* src, const int32_t* parents, int n_src, int n_dst, int64_t per_cand, float a,
                float b, uint64_t seed, uint32_t stream_id, int64_t cand_offset, void* stream) {
  if (!dst || !src || !parents) return fail(ITSD_ERR_INVALID, "itsd_branch: null argument");
  if (n_src < 1 || n_dst < 0 || per_cand < 1)
    return fail(ITSD_ERR_INVALID, "itsd_branch: needs n_src >= 1, n_dst >= 0, per_cand >= 1");
  if (n_dst == 0) return ITSD_OK;
  for (int j = 0; j < n_dst; ++j)
    if (parents[j] < 0 || parents[j] >= n_src)
      return fail(ITSD_ERR_INVALID, "itsd_branch: parents[" + std::to_string(j) + "] = " + std::to_string(parents[j]) +
                                        " outside [0, n_src=" + std::to_string(n_src) + ")");
  {
    const uintptr_t d0 = (uintptr_t)dst, s0 = (uintptr_t)src;
    const uintptr_t db = (uintptr_t)n_dst * (uintptr_t)per_cand * 4, sb = (uintptr_t)n_src * (uintptr_t)per_cand * 4;
    if (d0 < s0 + sb && s0 < d0 + db) return fail(ITSD_ERR_INVALID, "itsd_branch: dst and src overlap");
  }
  HIPCHK(launch_branch(dst, src, parents, n_dst, per_cand, a, b, seed, stream_id, cand_offset, (hipStream_t)stream));
  return ITSD_OK;
}

int itsd_verify(int kind, const float* images, int n_cand, int b, int c, int h, int w, double* scores, void* stream) {
  if (!images || !scores || n_cand < 1 || b < 1) return fail(ITSD_ERR_INVALID, "bad verify arguments");
  if (kind < 0 || kind > 3) return fail(ITSD_ERR_INVALID, "unknown verifier kind");
  if (kind == ITSD_VERIFY_SELFSUP && (c * 64 > 192 || h % 8 || w % 8 || b > 64))
    return fail(ITSD_ERR_INVALID, "selfsup verifier needs c<=3, h,w divisible by 8, b<=64");
  HIPCHK(launch_verify(kind, images, n_cand, b, c, h, w, scores, nullptr, (hipStream_t)stream));
  return ITSD_OK;
}

int itsd_verify_paired(const float* images, const float* ref_features, int n_cand, int c, int h, int w,
                       double* scores, void* stream) {
  if (!images || !ref_features || !scores || n_cand < 1) return fail(ITSD_ERR_INVALID, "bad verify arguments");
  if (c * 64 > 192 || h % 8 || w % 8) return fail(ITSD_ERR_INVALID, "paired selfsup needs c<=3, h,w divisible by 8");
  HIPCHK(launch_verify(4, images, n_cand, 1, c, h, w, scores, ref_features, (hipStream_t)stream));
  return ITSD_OK;
}

int itsd_attention(const void* qkv, const void* vt, void* out, int n, int S, int C, int precision, void* stream) {
  if (!qkv || !out || n < 1 || S < 1 || C < 1) return fail(ITSD_ERR_INVALID, "bad attention arguments");
  if (precision != ITSD_PREC_FP32 && precision != ITSD_PREC_BF16) return fail(ITSD_ERR_INVALID, "precision");
  AttnArgs a{};
  a.qkv = qkv; a.out = out; a.S = S; a.C = C;
  a.scale = (float)std::pow((double)C, -0.5);
  if (precision == ITSD_PREC_BF16) {
    if (C % 8) return fail(ITSD_ERR_INVALID, "C must be a multiple of 8");
    if (vt) {
      if (S % 16 || C % 64 || (S > 256 && !attn_flash_ok(S, C) && !attn_cs_ok(S, C)))
        return fail(ITSD_ERR_INVALID, "MFMA attention needs S % 16 == 0, C % 64 == 0 (S > 256: S % 32 == 0 with C in "
                                      "{64,128,256}, or S % 64 == 0 with C in {256,384,512,1024})");
      a.vt = vt;
    }
    HIPCHK(launch_attn<bf16_t>(a, n, (hipStream_t)stream));
  } else {
    if (C % 4) return fail(ITSD_ERR_INVALID, "C must be a multiple of 4");
    HIPCHK(launch_attn<float>(a, n, (hipStream_t)stream));
  }
  return ITSD_OK;
}

int itsd_noise(float* out, const float* pivot, int n_cand, int64_t per_cand, float scale, uint64_t seed,
               uint32_t stream_id, int64_t cand_offset, void* stream) {
  if (!out || n_cand < 0 || per_cand < 1) return fail(ITSD_ERR_INVALID, "bad noise arguments");
  if (n_cand == 0) return ITSD_OK;
  HIPCHK(launch_noise(out, pivot, n_cand, per_cand, scale, seed, stream_id, cand_offset, (hipStream_t)stream));
  return ITSD_OK;
}

namespace {
constexpr int64_t kEsMaxPer = (int64_t)1 << 40;  // es_adam_kernel's blocks fit gridDim.x, the workspace size an int64
bool es_sizes_ok(int n_pairs, int64_t per_cand) {
  return n_pairs >= 1 && n_pairs <= kEsMaxPairs && per_cand >= 1 && per_cand <= kEsMaxPer;
}
}  // namespace

int64_t itsd_es_workspace_bytes(int n_pairs, int64_t per_cand) {
  return es_sizes_ok(n_pairs, per_cand) ? (int64_t)es_workspace_bytes(n_pairs, per_cand) : 0;
}

int itsd_es_candidates(float* out, const float* pivot, int n_cand, int64_t per_cand, float sigma, uint64_t seed,
                       uint32_t stream_id, int64_t cand_offset, void* stream) {
  if (!out || !pivot) return fail(ITSD_ERR_INVALID, "itsd_es_candidates: null argument");
  if (n_cand < 0 || per_cand < 1 || per_cand > kEsMaxPer || cand_offset < 0)
    return fail(ITSD_ERR_INVALID, "itsd_es_candidates: needs n_cand >= 0, 1 <= per_cand <= 2^40, cand_offset >= 0");
  if (!std::isfinite(sigma) || sigma <= 0.0f)
    return fail(ITSD_ERR_INVALID, "itsd_es_candidates: sigma must be finite and > 0");
  if (n_cand == 0) return ITSD_OK;
  HIPCHK(launch_es_candidates(out, pivot, n_cand, per_cand, sigma, seed, stream_id, cand_offset, (hipStream_t)stream));
  return ITSD_OK;
}

int itsd_es_step(float* theta, float* m, float* v, const float* w, int n_pairs, int64_t per_cand, uint64_t seed,
                 uint32_t stream_id, const itsd_adam_step* adam, float* grad_out, double* gnorm2_out, void* ws,
                 void* stream) {
  if (!theta || !m || !v || !w || !adam || !gnorm2_out || !ws)
    return fail(ITSD_ERR_INVALID, "itsd_es_step: null argument");
  if (!es_sizes_ok(n_pairs, per_cand))
    return fail(ITSD_ERR_INVALID, "itsd_es_step: needs 1 <= n_pairs <= " + std::to_string(kEsMaxPairs) +
                                      ", 1 <= per_cand <= 2^40");
  if ((uintptr_t)ws % 16) return fail(ITSD_ERR_INVALID, "itsd_es_step: ws must be 16-byte aligned");
  const float f[7] = {adam->beta1, adam->omb1, adam->beta2, adam->omb2, adam->c1, adam->c2, adam->eps};
  for (float x : f)
    if (!std::isfinite(x)) return fail(ITSD_ERR_INVALID, "itsd_es_step: a field of adam is not finite");
  if (adam->beta1 < 0.0f || adam->beta1 >= 1.0f || adam->beta2 < 0.0f || adam->beta2 >= 1.0f)
    return fail(ITSD_ERR_INVALID, "itsd_es_step: adam beta1 / beta2 must lie in [0, 1)");
  if (adam->eps <= 0.0f) return fail(ITSD_ERR_INVALID, "itsd_es_step: adam eps must be > 0");
  {
    const uintptr_t eb = (uintptr_t)per_cand * 4;
    const struct { const char* name; uintptr_t p, bytes; } r[5] = {
        {"theta", (uintptr_t)theta, eb}, {"m", (uintptr_t)m, eb}, {"v", (uintptr_t)v, eb},
        {"grad_out", (uintptr_t)grad_out, eb}, {"ws", (uintptr_t)ws, (uintptr_t)es_workspace_bytes(n_pairs, per_cand)}};
    for (int i = 0; i < 5; ++i)
      for (int j = i + 1; j < 5; ++j)
        if (r[i].p && r[j].p && r[i].p < r[j].p + r[j].bytes && r[j].p < r[i].p + r[i].bytes)
          return fail(ITSD_ERR_INVALID, std::string("itsd_es_step: ") + r[i].name + " and " + r[j].name + " overlap");
  }
  const EsAdam a{adam->beta1, adam->omb1, adam->beta2, adam->omb2, adam->c1, adam->c2, adam->eps};
  HIPCHK(launch_es_step(theta, m, v, w, n_pairs, per_cand, seed, stream_id, a, grad_out, gnorm2_out, ws,
                        (hipStream_t)stream));
  return ITSD_OK;
}

int itsd_profile_forward(itsd_unet* u, const float* x, const int32_t* t, int n, double* conv_ms, double* conv_flops,
                         int* conv_launches, double* total_ms, void* stream) {
  if (!u || !x || !t) return fail(ITSD_ERR_INVALID, "null argument");
  if (u->cfg) return fail(ITSD_ERR_INVALID, "profile_forward: DDPM only");
  hipStream_t s = u->stream;
  ProfileScratch p;
  CHK(p.begin(u, t, n, (hipStream_t)stream));
  RunCtx c = forward_ctx(u, n, x, nullptr, p.eps);
  p.census(c, false);
  int r = run_program(u, c, resolve_program(u, c), s);
  hipError_t e = hipStreamSynchronize(s);
  CHK(r);
  HIPCHK(e);
  double cm = 0, cf = 0, tm = 0;
  int cl = 0;
  for (size_t i = 0; i < p.evs.size(); ++i) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, p.evs[i].first, p.evs[i].second);
    tm += ms;
    if (p.kinds[i] == OP_CONV || p.kinds[i] == kCensusConvGN || p.kinds[i] == kCensusConvGNW ||
        p.kinds[i] == kCensusConvGNW4) {
      cm += ms; cf += p.fl[i]; ++cl;
    }
  }
  if (conv_ms) *conv_ms = cm;
  if (conv_flops) *conv_flops = cf;
  if (conv_launches) *conv_launches = cl;
  if (total_ms) *total_ms = tm;
  return ITSD_OK;
}

int itsd_profile_op(itsd_unet* u, const float* x, const int32_t* t, int n, int op_index, int reps, double* ms,
                    void* stream) {
  if (!u || !x || !t || !ms || reps < 1) return fail(ITSD_ERR_INVALID, "null argument or reps < 1");
  if (op_index < 1 || op_index > (int)u->ops.size()) return fail(ITSD_ERR_INVALID, "profile_op: op_index out of range");
  hipStream_t s = u->stream;
  ProfileScratch p;
  CHK(p.begin(u, t, n, (hipStream_t)stream));
  const RunCtx c = forward_ctx(u, n, x, p.lab0, p.eps);
  const std::vector<ConvLaunch> convs = resolve_program(u, c);
  CHK(run_program(u, c, convs, s));  // every op's inputs in place
  p.evs.push_back({nullptr, nullptr});
  hipEvent_t &e0 = p.evs[0].first, &e1 = p.evs[0].second;
  HIPCHK(hipEventCreate(&e0));
  HIPCHK(hipEventCreate(&e1));
  const Op& o = u->ops[op_index - 1];
  const ConvLaunch* cl = &convs[op_index - 1];
  CHK(launch_op(u, o, c, cl, s));  // warm
  HIPCHK(hipEventRecord(e0, s));
  for (int i = 0; i < reps; ++i) CHK(launch_op(u, o, c, cl, s));
  HIPCHK(hipEventRecord(e1, s));
  HIPCHK(hipStreamSynchronize(s));
  float m = 0.f;
  HIPCHK(hipEventElapsedTime(&m, e0, e1));
  *ms = (double)m / reps;
  return ITSD_OK;
}

int itsd_profile_ops(itsd_unet* u, const float* x, const int32_t* t, int n, int max_ops, int* kinds, double* ms,
                     double* flops, int* shapes, int* n_ops, void* stream) {
  if (!u || !x || !t || !n_ops) return fail(ITSD_ERR_INVALID, "null argument");
  hipStream_t s = u->stream;
  ProfileScratch p;
  CHK(p.begin(u, t, n, (hipStream_t)stream));
  RunCtx c = forward_ctx(u, n, x, p.lab0, p.eps);
  p.census(c, true);
  const std::vector<ConvLaunch> convs = resolve_program(u, c);
  int r = run_program(u, c, convs, s);
  hipError_t e = hipStreamSynchronize(s);
  CHK(r);
  HIPCHK(e);
  // launch order: head, ops..., tail GN, tail
  int k = 0;
  for (size_t i = 0; i < p.evs.size() && k < max_ops; ++i, ++k) {
    const int op = p.eop[i];
    float m = 0.f;
    hipEventElapsedTime(&m, p.evs[i].first, p.evs[i].second);
    if (kinds) kinds[k] = (p.kid[i] << 8) | (p.kinds[i] & 0xff);
    if (ms) ms[k] = m;
    if (flops) flops[k] = p.fl[i];
    if (shapes) {
      int* sh = shapes + 8 * k;
      for (int q = 0; q < 8; ++q) sh[q] = 0;
      sh[6] = op;
      if (op >= 1) {
        const Op& o = u->ops[op - 1];
        const Act& out = u->acts[o.dst >= 0 ? o.dst : o.src1];
        const Act& in = u->acts[o.src1];
        sh[0] = n * out.H * out.W;
        sh[1] = o.kind == OP_CONV ? o.Cout : out.C;
        sh[2] = o.kind == OP_CONV ? o.K : in.C + (o.src2 >= 0 ? u->acts[o.src2].C : 0);
        sh[3] = out.H;
        sh[4] = o.ksize;
        sh[5] = o.stride * 10 + o.upsample;
        // flags for the algorithmic-bytes count (bench.py conv_alg_bytes): bit 0 a residual operand, bit 1 the
        // output's GroupNorm statistics written, bit 2 the input GroupNorm(+SiLU) fused (its statistics read)
        sh[7] = (o.resid >= 0 ? 1 : 0) | (out.stats != SIZE_MAX ? 2 : 0) | (o.coef != SIZE_MAX ? 4 : 0);
        // a block2 conv with its 1x1 shortcut folded in as K slices: no residual operand; the shortcut's input
        // channels in bits 8..
        const ConvLaunch& cl = convs[op - 1];
        if (cl.p.sc_split) sh[7] = (sh[7] & ~1) | ((cl.a.sc_C1 + cl.a.sc_C2) << 8);
      }
    }
  }
  *n_ops = k;
  return ITSD_OK;
}

// ---- introspection of the op program (include/itsd.h): eager host code beside the program, nothing on its path
int itsd_unet_op_info(itsd_unet* u, int pass, int n, int op_index, itsd_op_info* info) {
  if (!u || !info) return fail(ITSD_ERR_INVALID, "null argument");
  if (pass != ITSD_PASS_FORWARD && pass != ITSD_PASS_STEP) return fail(ITSD_ERR_INVALID, "op_info: unknown pass");
  const int nops = (int)u->ops.size();
  if (op_index < 0 || op_index > nops + 1)
    return fail(ITSD_ERR_INVALID, "op_info: op_index outside [0, ops + 1 = " + std::to_string(nops + 1) + "]");
  CHK(check_batch(u, n));
  itsd_op_info r;
  std::memset(&r, 0, sizeof(r));
  r.launched = 1;
  r.src1 = r.src2 = r.dst = r.resid = r.vt = r.temb_col = r.kernel = -1;
  auto name = [&r](const std::string& s) { std::snprintf(r.name, sizeof(r.name), "%s", s.c_str()); };
  if (op_index == 0) {
    r.kind = ITSD_OP_HEAD;
    r.dst = u->head_out;
    r.ksize = 3; r.stride = 1; r.pad = 1; r.Cout = u->ch; r.K = 27;
    name("head");
  } else if (op_index == nops + 1) {
    r.kind = ITSD_OP_TAIL;
    r.src1 = u->tail_in;
    r.dst = u->tail_g;  // (the plain tail's GroupNorm output; -1: fused into tail_mfma_kernel through the coef buffer)
    r.has_coef = u->tail_wmf != SIZE_MAX;
    r.silu = 1;
    r.ksize = 3; r.stride = 1; r.pad = 1; r.Cout = 3; r.K = 9 * u->acts[u->tail_in].C;
    name("tail");
  } else {
    // a throw-away pass context: what itsd_unet_forward, or the sampler step (itsd_sampler_run / _predict_x0: the
    // doubled cond||uncond batch for CFG), resolves at this batch (no pointer in it is followed)
    const RunCtx c = pass == ITSD_PASS_STEP ? step_ctx(u, n, nullptr, nullptr) : forward_ctx(u, n, nullptr, nullptr, nullptr);
    const std::vector<ConvLaunch> rp = resolve_program(u, c);
    const int oi = op_index - 1;
    const Op& o = u->ops[oi];
    r.kind = o.kind == OP_GN ? ITSD_OP_GN : o.kind == OP_CONV ? ITSD_OP_CONV : o.kind == OP_ATTN ? ITSD_OP_ATTN
             : o.kind == OP_GNCOEF ? ITSD_OP_GNCOEF : ITSD_OP_ATTNBLOCK;
    r.src1 = o.src1; r.src2 = o.src2; r.dst = o.dst; r.resid = o.resid; r.vt = o.vt;
    r.silu = o.silu;
    r.S = o.S; r.C = o.C;
    r.tag = o.tag;
    name(o.name);
    if (const int into = folded_into(u, rp, (size_t)oi); into >= 0) { r.launched = 0; r.folded_into = into + 1; }
    if (o.kind == OP_GNCOEF) r.has_coef = 1;
    if (o.kind == OP_CONV) {
      const ConvLaunch& cl = rp[oi];
      if (cl.rc != ITSD_OK) return fail(cl.rc, cl.err);
      r.ksize = o.ksize; r.stride = o.stride; r.pad = o.pad; r.upsample = o.upsample; r.zins = o.zins;
      r.subpix = o.subpix; r.Cout = o.Cout; r.K = o.K; r.temb_col = o.temb_col; r.vt_from = o.vt_from;
      r.kernel = (int)cl.p.kernel;
      r.ksplit = cl.p.ksplit; r.sc_split = cl.p.sc_split; r.kS = cl.p.S;
      r.epilogue = cl.p.epilogue ? 1 : 0;
      r.gn_fold = cl.a.gn_fold;
      r.gn_out_op = cl.a.gn_out ? o.gn_next + 1 : 0;
      r.sc_op = cl.p.sc_split ? o.sc_op + 1 : 0;
      r.has_coef = o.coef != SIZE_MAX;
    }
  }
  *info = r;
  return ITSD_OK;
}

int itsd_unet_act_info(const itsd_unet* u, int act, itsd_act_info* info) {
  if (!u || !info) return fail(ITSD_ERR_INVALID, "null argument");
  itsd_act_info r;
  std::memset(&r, 0, sizeof(r));
  if (act == ITSD_ACT_PROJ) {
    r.H = r.W = 1; r.C = u->sumC; r.elem_size = 4; r.capacity = u->d.max_batch;
  } else {
    if (act < 0 || act >= (int)u->acts.size())
      return fail(ITSD_ERR_INVALID, "act_info: act outside [0, " + std::to_string(u->acts.size()) + ")");
    const Act& A = u->acts[act];
    r.H = A.H; r.W = A.W; r.C = A.C; r.elem_size = (int)u->esz; r.capacity = u->nb_max;
    r.has_stats = A.stats != SIZE_MAX;
    r.spi = stat_spi(A.H * A.W, A.spi);
  }
  *info = r;
  return ITSD_OK;
}

int itsd_unet_read(itsd_unet* u, int what, int id, int n, void* dst, int64_t bytes, void* stream) {
  if (!u || !dst) return fail(ITSD_ERR_INVALID, "null argument");
  const char* src = nullptr;
  int64_t want = 0;
  int cap = u->nb_max;
  if (what == ITSD_READ_ACT || what == ITSD_READ_STATS) {
    if (id < 0 || id >= (int)u->acts.size())
      return fail(ITSD_ERR_INVALID, "read: act outside [0, " + std::to_string(u->acts.size()) + ")");
    const Act& A = u->acts[id];
    if (what == ITSD_READ_ACT) {
      src = u->ws + A.off;
      want = (int64_t)A.H * A.W * A.C * (int64_t)u->esz;
    } else {
      if (A.stats == SIZE_MAX) return fail(ITSD_ERR_INVALID, "read: activation " + std::to_string(id) + " has no statistics slab");
      src = u->ws + A.stats;
      want = (int64_t)stat_spi(A.H * A.W, A.spi) * 2 * A.C * 4;
    }
  } else if (what == ITSD_READ_COEF) {
    const int nops = (int)u->ops.size();
    if (id == nops + 1 && u->tail_coef != SIZE_MAX) {
      src = u->ws + u->tail_coef;
      want = (int64_t)u->acts[u->tail_in].C * 2 * 4;
    } else if (id >= 1 && id <= nops && u->ops[id - 1].kind == OP_GNCOEF) {
      const Op& o = u->ops[id - 1];
      src = u->ws + o.coef;
      want = (int64_t)(u->acts[o.src1].C + (o.src2 >= 0 ? u->acts[o.src2].C : 0)) * 2 * 4;
    } else {
      return fail(ITSD_ERR_INVALID, "read: op " + std::to_string(id) + " has no coef buffer");
    }
  } else if (what == ITSD_READ_PROJ) {
    src = (const char*)u->proj_buf;
    want = (int64_t)u->sumC * 4;
    cap = u->d.max_batch;
  } else {
    return fail(ITSD_ERR_INVALID, "read: unknown buffer class " + std::to_string(what));
  }
  if (n < 1 || n > cap) return fail(ITSD_ERR_INVALID, "read: n outside [1, " + std::to_string(cap) + "]");
  want *= n;
  if (bytes != want)
    return fail(ITSD_ERR_INVALID, "read: bytes = " + std::to_string(bytes) + ", the buffer holds " + std::to_string(want));
  hipStream_t cs = (hipStream_t)stream;
  CHK(enter_stream(u, cs));
  HIPCHK(hipMemcpyAsync(dst, src, (size_t)want, hipMemcpyDeviceToDevice, u->stream));
  return leave_stream(u, cs);
}

int itsd_unet_poison(itsd_unet* u, void* stream) {
  if (!u) return fail(ITSD_ERR_INVALID, "null argument");
  hipStream_t cs = (hipStream_t)stream;
  CHK(enter_stream(u, cs));
  // the arena holds activations, channel-major V, coef buffers and statistics slabs only (Builder::act, conv_layer,
  // build): all of them stored whole by their producers
  HIPCHK(hipMemsetAsync(u->ws, 0xFF, u->ws_bytes, u->stream));
  HIPCHK(hipMemsetAsync(u->splitk_ws, 0xFF, (size_t)itsd_unet::kSplitkCap * 4, u->stream));
  // itsd_verify_denoise's scratch (once it exists): the call stores every element it reads
  if (u->vd_xt) HIPCHK(hipMemsetAsync(u->vd_xt, 0xFF, vd_xt_bytes(u), u->stream));
  if (u->vd_part) HIPCHK(hipMemsetAsync(u->vd_part, 0xFF, vd_part_bytes(u), u->stream));
  // the traced step's per-block partials (once they exist): the tail stores every one its finalize launch reads
  if (u->tr_part) HIPCHK(hipMemsetAsync(u->tr_part, 0xFF, tr_part_bytes(u), u->stream));
  // the 2M step's x0 history (once it exists): a restarted run reads none of it, a continued one what the run before
  // it stored (the host's hist_row / hist_n stay: poisoning is a test of that claim, not an invalidation)
  if (u->x0_hist) HIPCHK(hipMemsetAsync(u->x0_hist, 0xFF, vd_xt_bytes(u), u->stream));
  u->last_forward_n = 0;  // (the tail input is gone: itsd_unet_representation refuses until the next forward)
  return leave_stream(u, cs);
}

}  // extern "C"
