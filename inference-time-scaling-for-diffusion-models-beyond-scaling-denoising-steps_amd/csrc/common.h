// Shared device helpers and kernel argument structs for libitsd_hip (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace itsd {

extern int g_conv_variant;  // kernel-variant switch for A/B measurements (itsd_set_option)
extern int g_small_conv;   // 64x64-tile conv_small for small levels (itsd_set_option "small_conv")
extern int g_splitk;        // split-K on/off (itsd_set_option "splitk")
extern int g_conv_dbg;      // measurement-only conv switches (itsd_set_option "conv_dbg")
extern int g_gn_wide;       // 256-pixel fused GroupNorm conv (itsd_set_option "gn_wide")
extern int g_attn_cs;       // attention output-channel slices (itsd_set_option "attn_cs")
extern int g_attn_aq;       // attention queries per block (itsd_set_option "attn_aq")
extern int g_p4_w;          // conv3x3_gn_p4_kernel level mask (itsd_set_option "p4_w")
extern int g_num_cus;       // compute units of the device (persistent grids)
extern int g_splitk_inl;     // conv_pipe split-K combined in-launch: 0 off (second launch), 1 on (itsd_set_option "splitk_inl")
extern int g_p4_plain;      // plain (no GroupNorm) 3x3 stride-1 convs on conv3x3_gn_p4_kernel<W, 2>: 0 off, 1 on (itsd_set_option "p4_plain")
extern int g_conv1x1;        // streaming 1x1 conv kernel: 0 off, 1 on ("conv1x1")
extern int g_small_8x8;      // conv_small (split K) for under-filled 8x8-level convs ("small_8x8")
extern int g_small_wide;     // conv_small for under-filled statistics-free convs of larger images ("small_wide")
extern int g_attn_wide_nq;   // its query groups a block: 0 auto, 1 / 2 forced ("attn_wide_nq")
extern int g_attn_wide;      // channel-split attention: 0 off, 1 auto, 2 wherever it applies ("attn_wide")
extern int g_small_minks;  // conv_small split K: >= this many K-chunks a slice ("small_minks")
extern int g_convt_prune;  // ConvTranspose2d sub-pixel phases skip their all-zero taps: 0 off, 1 on ("convt_prune")
extern int g_subpix_split;  // under-filled sub-pixel conv_pipe launches split K in-launch: 0 off, 1 on ("subpix_split")
extern int g_p4_xcd;        // persistent fused convs: contiguous tile ranges per XCD ("p4_xcd")
extern int g_p4_c96;        // 8x8 conv3x3_gn_p4_kernel<8, 512> (96-cout tiles): 0 off, 1 auto, 2 always (itsd_set_option "p4_c96")
extern int g_p4_sub;        // nearest-x2 upsample convs on conv3x3_gn_p4_kernel<W, 128>: 0 off, 1 on (itsd_set_option "p4_sub")
extern int g_p5;            // small-level fused conv conv3x3_gn_p5_kernel: 0 off (W = 8), 1 auto, 2 forced (itsd_set_option "p5")
extern int g_p5_split;      // its K slices: 0 auto (cost model), >= 1 forced (itsd_set_option "p5_split")
extern int g_p5_sc;         // 1x1 shortcut folded into the block2 p5 conv: 0 off, 1 auto, 2 always ("p5_sc")
extern int g_p5_xl;         // p5's split-K partials exchanged through one XCD's L2 (ConvArgs::kxl): 0 off, 1 / 2 / 3 (shipped) forms ("p5_xl")
extern int g_p5_pub;        // p5's two-slice combine: only the first arriver stores its partial: 0 off, 1 on ("p5_pub")
extern int g_p5_dist;       // p5 split-K combine by every slice where the grid is co-resident: 0 off, 1 on ("p5_dist")
extern int g_p5_c64;        // 64-cout p5 items at the 8x8 / 4x4 levels: 0 off, 1 auto, 2 always ("p5_c64", diagnostic)
extern int g_spin_bound;     // polls before an in-kernel hand-off wait fails: ITSD_ERR_HANDOFF ("spin_bound", diagnostic)
extern int g_attn_split;     // attn_block_split_kernel at small batches: 0 off, 1 auto, 2/4/6 forced G (itsd_set_option "attn_split")
extern int g_gn_fold;       // GroupNorm finalize inside p4 / p5 instead of a gn_coef launch (itsd_set_option "gn_fold")
extern int g_fuse_gn;       // fused GroupNorm+SiLU+conv3x3 in ResBlocks (itsd_set_option "fuse_gn", read at create)
// Census (itsd_profile_ops): the first kernel an op launches. Every launch site goes through
// ITSD_LAUNCH, which records the kernel expression's name if none is recorded yet; the census
// clears it before each op and maps the name to a small id (kernel_id, itsd_kernel_name).
// Per thread (a census on one thread never reads another thread's launches); kernel_id's
// registry is guarded by a mutex.
extern thread_local const char* g_last_kernel;
int kernel_id(const char* name);
#define ITSD_LAUNCH(K, ...)                                    \
  do {                                                         \
    if (!::itsd::g_last_kernel) ::itsd::g_last_kernel = #K;    \
    hipLaunchKernelGGL(K, __VA_ARGS__);                        \
  } while (0)

typedef uint16_t bf16_t;  // storage type for bf16 activations / weights

// In-launch split-K tickets per UNet handle: the hipMalloc'd counter array (api.hip itsd_unet::tickets)
// and every launch-side bound on ticket indices (conv.hip: conv_pipe / conv_small tile, p5 tile * 4 + wave)
// use this one constant.
constexpr long long kTicketCap = 16384;

// nn.GroupNorm(32, C, eps=1e-5) (Model.py:132,171,180,253): the host's GNArgs::eps and group arithmetic, and
// conv_small's fused GroupNorm epilogue
constexpr int kGnGroups = 32;
constexpr float kGnEps = 1e-5f;

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

__device__ __forceinline__ float bf2f(bf16_t u) { return __uint_as_float(((uint32_t)u) << 16); }
__device__ __forceinline__ bf16_t f2bf(float f) {
  __bf16 b = (__bf16)f;  // v_cvt_pk_bf16_f32: RNE, NaN stays NaN
  return __builtin_bit_cast(bf16_t, b);
}

// two floats -> one word of two bf16 (lo in the low half): one v_cvt_pk_bf16_f32
__device__ __forceinline__ uint32_t pk_bf16(float lo, float hi) {
  typedef float f2v __attribute__((ext_vector_type(2)));
  typedef __bf16 b2v __attribute__((ext_vector_type(2)));
  const b2v r = __builtin_convertvector((f2v){lo, hi}, b2v);
  return __builtin_bit_cast(uint32_t, r);
}

template <typename T> struct Elem;
template <> struct Elem<float> {
  static __device__ __forceinline__ float load(const float* p) { return *p; }
  static __device__ __forceinline__ float to(float v) { return v; }
  static __device__ __forceinline__ float tof(float v) { return v; }
};
template <> struct Elem<bf16_t> {
  static __device__ __forceinline__ float load(const bf16_t* p) { return bf2f(*p); }
  static __device__ __forceinline__ bf16_t to(float v) { return f2bf(v); }
  static __device__ __forceinline__ float tof(bf16_t v) { return bf2f(v); }
};

__device__ __forceinline__ float silu(float x) { return x / (1.0f + __expf(-x)); }

// Wave64 reductions.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// ----------------------------------------------------------------------------- register-epilogue pieces
// The MFMA kernels that write bf16 straight from their 32x32 accumulators (conv3x3_gn_p4 / p5_kernel,
// head_mfma_kernel, the AttnBlock's attn_out_tile) share these: lane (rl, hh) of a wave holds pixel rl and, per
// register group g, couts 8 g + 4 hh + 0..3. Every consumer-GroupNorm statistic they write goes through the one
// tree below, which is why their sums agree to the bit. The helpers take values and array references and hold no
// state between calls.

// the value of lane ^ W: DPP within a row (W = 1, 2, 8), ds_swizzle otherwise
template <int W> __device__ __forceinline__ float lane_xchg(float x) {
  const int xi = __builtin_bit_cast(int, x);
  int r;
  if constexpr (W == 1) r = __builtin_amdgcn_update_dpp(0, xi, 0xB1, 0xF, 0xF, false);
  else if constexpr (W == 2) r = __builtin_amdgcn_update_dpp(0, xi, 0x4E, 0xF, 0xF, false);
  else if constexpr (W == 8) r = __builtin_amdgcn_update_dpp(0, xi, 0x128, 0xF, 0xF, false);
  else r = __builtin_amdgcn_ds_swizzle(xi, 0x1F | (W << 10));
  return __builtin_bit_cast(float, r);
}
// One halving step over v[0..N): lanes with bit D of rl keep the upper N / 2 values, the others the lower, each
// summed with the partner lane's (rl ^ D) -> v[0..N / 2)
template <int D, int N> __device__ __forceinline__ void stat_halve(float (&v)[32], int rl) {
  const bool up = (rl & D) != 0;
#pragma unroll
  for (int i = 0; i < N / 2; ++i) {
    const float lo = v[i], hi = v[i + N / 2];
    v[i] = (up ? hi : lo) + lane_xchg<D>(up ? lo : hi);
  }
}
// 32 values a lane (16 sums, 16 sums of squares) over the 32 lanes of a pixel block -> one a lane: lane rl ends
// with v[0] = value index rl (rl < 16: the sum of cout 8 (e >> 2) + 4 hh + (e & 3), e = rl & 15; else its square sum)
__device__ __forceinline__ void stat_butterfly32(float (&v)[32], int rl) {
  stat_halve<16, 32>(v, rl);
  stat_halve<8, 16>(v, rl);
  stat_halve<4, 8>(v, rl);
  stat_halve<2, 4>(v, rl);
  stat_halve<1, 2>(v, rl);
}
__device__ __forceinline__ void stat_gather(float (&v)[32], const float (&s16)[16], const float (&q16)[16]) {
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    v[e] = s16[e];
    v[16 + e] = q16[e];
  }
}
// Register group g of one pixel block: acc + addv (+ the residual's four bf16, RES), rounded to bf16 once ->
// wv[g][0..1]; the rounded values (0 for a pixel that is not live) join the sums s16 / square sums q16
template <bool RES = true>
__device__ __forceinline__ void epi_frag(int g, float a0, float a1, float a2, float a3, f32x4 ad, uint2 rr, bool live,
                                         uint32_t (&wv)[4][2], float (&s16)[16], float (&q16)[16]) {
  const float v0 = RES ? a0 + ad[0] + __uint_as_float(rr.x << 16) : a0 + ad[0];
  const float v1 = RES ? a1 + ad[1] + __uint_as_float(rr.x & 0xffff0000u) : a1 + ad[1];
  const float v2 = RES ? a2 + ad[2] + __uint_as_float(rr.y << 16) : a2 + ad[2];
  const float v3 = RES ? a3 + ad[3] + __uint_as_float(rr.y & 0xffff0000u) : a3 + ad[3];
  const bf16_t b0 = f2bf(v0), b1 = f2bf(v1), b2 = f2bf(v2), b3 = f2bf(v3);
  wv[g][0] = (uint32_t)b0 | ((uint32_t)b1 << 16);
  wv[g][1] = (uint32_t)b2 | ((uint32_t)b3 << 16);
  const float m = live ? 1.0f : 0.0f;
  const float r0 = bf2f(b0) * m, r1 = bf2f(b1) * m, r2 = bf2f(b2) * m, r3 = bf2f(b3) * m;
  s16[4 * g + 0] += r0; q16[4 * g + 0] = fmaf(r0, r0, q16[4 * g + 0]);
  s16[4 * g + 1] += r1; q16[4 * g + 1] = fmaf(r1, r1, q16[4 * g + 1]);
  s16[4 * g + 2] += r2; q16[4 * g + 2] = fmaf(r2, r2, q16[4 * g + 2]);
  s16[4 * g + 3] += r3; q16[4 * g + 3] = fmaf(r3, r3, q16[4 * g + 3]);
}
// Register groups gp, gp + 1 (gp = 0, 2) of both half-waves -> this lane's 16 B: couts 8 (gp + hh) + 0..7 of its pixel
__device__ __forceinline__ u32x4 epi_pack(const uint32_t (&wv)[4][2], int gp) {
  u32x4 o;
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const auto sw = __builtin_amdgcn_permlane32_swap(wv[gp][d], wv[gp + 1][d], false, false);
    o[d] = sw[0];
    o[2 + d] = sw[1];
  }
  return o;
}

// ----------------------------------------------------------------------------- args
// Implicit-GEMM convolution over NHWC activations (see conv.hip).
struct ConvArgs {
  const void* src1;  // [n][Hin][Win][C1]
  const void* src2;  // [n][Hin][Win][C2] (channel-concat second source, Model.py:280) or null
  int C1, C2;
  int Hin, Win, Hout, Wout;
  int ksize, stride, pad, upsample;  // upsample: nearest x2 folded into addressing (Model.py:123)
  int zins;                          // zero-insertion (ConvTranspose2d s2 as a gather conv, ModelCondition.py:80)
  const void* wt;                    // packed [Cout][K], K = ksize*ksize*(C1+C2), k=(ky*ks+kx)*Cin+ci
  const void* wfrag;                 // the same weights in MFMA A-fragment order [Cout/32][K/16][64][8]
  int Cout, K;
  const float* bias;                 // [Cout]
  // epilogue additive vectors (ResBlock temb_proj, Model.py:204; CFG cond_proj ModelCondition.py:156)
  const float* temb;                 // temb[(tsel? *tsel*row : 0) + img*img_stride + co]
  const int* temb_tsel;
  long long temb_row_stride, temb_img_stride;
  const float* cemb;                 // cemb[labels[img]*row + co]
  const int* cemb_labels;
  long long cemb_row_stride;
  int cemb_label_mod;                // labels index = img % mod (CFG cond||uncond batch)
  int cemb_uncond_from;              // images >= this use label 0 (uncond half); <0 disables
  const void* resid;                 // [M][Cout] same layout as out, or null
  void* out;                         // [M][Cout]
  int M;                             // n * Hout * Wout
  float* stats;                      // channel-statistics slab [slot][2][Cout] for the consumer GN, or null
  const void* zero;                  // >= 16 zero bytes: DMA source for padded / out-of-range rows
  void* vt_out;                      // couts >= vt_from go channel-major to vt_out[img][co-vt_from][HWo]
  int vt_from;                       // (the V of a fused q|k|v projection, for the MFMA attention)
  float* splitk_ws;                  // split-K partial tiles (capacity splitk_cap floats) or null
  long long splitk_cap;
  // fused GroupNorm+SiLU of the input (bf16 3x3, conv3x3_gn_kernel): per-image channel
  // coefficients coef[img][Cin/8][a0..a7, b0..b7] (gn_coef_kernel); null = plain conv
  const float* gn_coef;
  int subpix;                        // 1: nearest-x2 upsample + 3x3 conv run as 4 phase-wise 2x2 convs;
                                     // 2: ConvTranspose2d(5, 2, 2, 1) as 4 phase-wise 3x3 convs (pad 1)
                                     // (grid.z = phase py*2+px): Hout/Wout/M/ksize/K describe the
                                     // input-grid GEMM; output rows are (2i+py, 2j+px) of a 2x grid
  int dbg;                           // g_conv_dbg (measurements only)
  int xcd;                           // persistent fused convs: deal each XCD a contiguous range of tiles (speed only)
  int tap_live;                      // subpix 2 on conv3x3_gn_p4_kernel: skip each phase's all-zero taps
                                     // (conv_pipe runs all 9: measured no faster with live taps)
  // conv3x3_gn_p5_kernel (the fused conv of the 8x8 / 4x4 levels): K split into ksplit slices
  // (>= 1) combined in-launch by the last-arriving slice of each (tile, MFMA wave); tickets[]
  // are zero between launches (zeroed at create, reset by each last arriver)
  int ksplit;
  int* tickets;
  // the GroupNorm finalize folded into conv3x3_gn_p4 / p5_kernel (gn_fold != 0: the gn_coef launch is
  // skipped and the halo waves reduce the input's statistics slabs to group mean / rstd themselves)
  int gn_fold;
  const float* gn_st1;
  const float* gn_st2;
  int gn_spi1, gn_spi2;
  const float* gn_gamma;
  const float* gn_beta;
  // conv3x3_gn_p5_kernel with the ResBlock's 1x1 shortcut folded in (Model.py:200-205, h + shortcut(x)):
  // sc_split more K slices after the ksplit 3x3 ones, over x = sc_src1 ++ sc_src2 (raw, no GroupNorm) with the
  // shortcut's fragment-ordered weights sc_wfrag [Cout/32][(sc_C1+sc_C2)/16][64][8]; bias = both biases summed,
  // resid = null. sc_split == 0: no shortcut slices
  const void* sc_src1;
  const void* sc_src2;
  int sc_C1, sc_C2, sc_split;
  const void* sc_wfrag;
  // conv3x3_gn_p5_kernel's split-K combine shared by all slices (kdist != 0: every block runs one item, so the
  // grid is co-resident): each slice waits for the tile's other slices and finishes its own share of the tile's
  // units; a wait that exhausts spin_bound polls sets bit 1 of *err and writes NaN (ITSD_ERR_HANDOFF)
  int kdist;
  // two slices, last-arriver form (kdist == 0, ST == 2): kpub != 0 -- arrival first, only the first arriver stores its
  // partial (sc1, drained, then publishes on the same counter), the last one adds it to its own from registers
  int kpub;
  // XCD-local split-K exchange (kdist or the two-slice kpub form): the slices of a tile are adjacent items, so they
  // run on blocks of one XCD (the dispatcher deals block b to XCD b % 8) and exchange partials through that XCD's
  // L2 -- plain stores, L1-bypassing (sc0) loads -- instead of writing through to memory (sc1). Each slice reports
  // its XCC_ID with its arrival; a tile whose slices ran on different XCDs is poisoned with NaN and sets bit 1 of
  // *err (ITSD_ERR_HANDOFF): never a silent stale read
  int kxl;
  int* err;
  int spin_bound;
  // conv_small (whole-image tiles, HWo <= 16) with its consumer GroupNorm(+SiLU) fused into the epilogue: the next op
  // (gn_apply_kernel over this output alone) is skipped and the epilogue writes silu(GN(out)) to gn_out as well, from
  // the same per-channel slot sums and the same fp64 group finalize (bit-identical); a group's channels lie inside
  // one 64-cout tile (host: 64 % (Cout / 32) == 0). Null: no fused GroupNorm
  void* gn_out;
  const float* go_gamma;
  const float* go_beta;
  int go_silu;
};

// How launch_conv runs one conv: every decision between the ConvArgs and the launch, made once by plan_conv (conv.hip,
// host only) and shared with the host program (api.hip: the GroupNorm / shortcut folds, the census).
enum class ConvKernel {
  P5,           // conv3x3_gn_p5_kernel<W>, split-K combined by each tile's last-arriving slice
  P5_SHARED,    // conv3x3_gn_p5_kernel<W, 128, true>: the combine shared by every slice (kdist)
  P4_GN,        // conv3x3_gn_p4_kernel<W>: fused GroupNorm, 256 pixels x 128 couts
  P4_C96,       // conv3x3_gn_p4_kernel<8, 512>: ... on 96-cout tiles
  P4_PLAIN,     // conv3x3_gn_p4_kernel<W, 2>: no GroupNorm
  P4_SUB,       // conv3x3_gn_p4_kernel<W, 128>: the 2x2-tap phases of a nearest-x2 upsample conv
  P4_CONVT,     // conv3x3_gn_p4_kernel<W, 384>: the 3x3-tap phases of ConvTranspose2d(5, 2, 2, 1)
  GN128,        // conv3x3_gn_kernel<gn_segs>: fused GroupNorm, 128 x 128 tiles
  STREAM1X1,    // conv1x1_stream_kernel<Cin, 4 | 7>
  SMALL,        // conv_small<false>: 64 x 64 tiles, grid.z K slices combined in-launch
  PIPE_LIN,     // conv_pipe<T, 2, true>: plain stride / pad addressing
  PIPE,         // conv_pipe<T, 2, false>: nearest-x2 upsample / zero insertion folded into the addressing
  PIPE_SUBPIX,  // conv_pipe<T, 2, true> over 4 sub-pixel phases (grid.z = 4 x K slices)
  IGEMM,        // conv_igemm<T>: register-staged fallback
};
struct ConvPlan {
  bool valid = true;  // false: a shape no kernel takes (launch_conv returns hipErrorInvalidValue)
  ConvKernel kernel = ConvKernel::IGEMM;
  dim3 grid;
  int block = 256;
  // p5 (copied into ConvArgs::ksplit / sc_split / kdist / kpub / kxl by launch_conv); cb: its cout tile (128; 64 in
  // diagnostic builds). sc_split > 0: the args' sc_* shortcut is folded in (0: the caller drops it and launches the
  // shortcut conv itself)
  int ksplit = 1, sc_split = 0, cb = 128, kdist = 0, kpub = 0, kxl = 0;
  // K slices of conv_small / conv_pipe (in grid.z). conv_pipe combines them in-launch on the args' tickets (inl) or,
  // without tickets, by a splitk_epilogue_kernel launch over grid.x x grid.y (epilogue)
  int S = 1;
  bool inl = true, epilogue = false;
  int gn_segs = 0;    // GN128: images a 128-pixel tile spans (1 | 2)
  int wide_segs = 0;  // fused GroupNorm convs: 1 rows of one image / 4 four 8x8 images a 256-pixel tile, 0 neither
                      // (the census kind)
};
ConvPlan plan_conv(const ConvArgs& a, bool bf16);

// Channel-statistics slab of an NHWC tensor (written by its producer): slots of
// Gt = min(HW, 128) consecutive pixels; stats[slot][0][c] = sum, [slot][1][c] = sum of squares.
__host__ __device__ inline int stat_slot_px(int HW) { return HW < 128 ? HW : 128; }
// Statistics slots per image of a tensor: HW / stat_slot_px(HW), except the output of a sub-pixel
// upsample conv whose phase images are smaller than a slot: one slot per (image, phase).
__host__ __device__ inline int stat_spi(int HW, int spi) { return spi > 0 ? spi : HW / stat_slot_px(HW); }

struct GNArgs {
  const void* src1; const void* src2;  // NHWC, C1 (+ C2) channels
  const float* st1; const float* st2;  // their statistics slabs
  int C1, C2, HW;
  int spi1, spi2;                      // statistics slots per image of src1 / src2 (0: HW / stat_slot_px(HW))
  const float* gamma; const float* beta;
  float eps;
  int silu;
  void* dst;                           // NHWC, C1+C2 channels
  int chunks_per_block;                // 16-B chunks of one image handled per block
};

struct AttnArgs {
  const void* qkv;  // [n][S][3C]  (q | k | v per token; v unused when vt != null)
  const void* vt;   // [n][C][S]   channel-major v (MFMA path) or null
  void* out;        // [n][S][C]
  int S, C;
  float scale;
};

// Fused AttnBlock at S = 64 (kernels.hip attn_block_kernel).
struct AttnBlockArgs {
  const bf16_t* x;        // [n][S][C] NHWC (the ResBlock output)
  const float* st;        // its GroupNorm statistics slab [n * spi][2][C]
  int spi;                // statistics slots per image
  const float* gamma; const float* beta;
  const bf16_t* wmv;      // [2C/32][C/16][64][8]: the folded M = Wq^T Wk rows, then the W' = (Wp Wv)^T rows
  const float* buv;       // [2C]: u = Wk^T bq | b' = Wp bv
  const float* bp;        // [C] the proj bias
  bf16_t* out;            // [n][S][C]
  float* out_stats;       // [n][2][C] (one slot per image) or null
  float scale;            // C^-0.5
  int n;
  int S;                  // tokens an image: 64 (one image a block) or 16 (4 images a block)
  // attn_block_split_kernel (an image's work over G blocks, small batches): the partial-score slab
  // (write-through hand-off) and one monotonic counter per image
  float* spart;           // [n][G][4 tiles][64 lanes][16] fp32
  int* sync;              // [n], never reset (targets from each block's own add)
  int* err;               // device status word: bit 0 set when a hand-off wait exhausted its poll bound
  int spin_bound;         // polls before a hand-off wait gives up (itsd_set_option "spin_bound", diagnostic)
};

struct HeadArgs {
  const float* x;       // NCHW fp32 [n][3][H][W]
  const float* w;       // [Cout][3][3][3] fp32 (reference layout)
  const float* b;
  void* out;            // NHWC [n][H][W][Cout]
  int H, W, Cout, n;
  int x_img_mod;        // image i reads x[i % x_img_mod] (CFG cond||uncond batch)
  float* stats;         // GroupNorm statistics slab of the output [slot][2][Cout], or null
  const bf16_t* wmf;    // bf16 MFMA weights [Cout][32] (k = ci*9 + tap, zero-padded 27..31), or null
};

// Per-run sampler parameters, kept in device memory so that one captured step graph serves
// every run of a search (only the values change between rounds, never the graph).
struct RunParams {
  unsigned long long seed;  // Philox key of the per-step noise z
  long long noise_offset;   // Philox element offset (global candidate index * per-candidate elements)
  int clip_at;              // clip when t == clip_at (-1: never)
  int restart_at;           // the 2M step at row t == restart_at has no history: it uses its own x0 twice (-1: none)
};
static_assert(sizeof(RunParams) == 24, "RunParams is the argument of run_begin_kernel and a device block: fixed");

// The eight ways the tail ends (TailArgs::step_mode; kernels.hip's header comment describes each). The values are the
// ABI of TailArgs and stay.
enum TailMode : int {
  kTailEps = 0,        // write eps NCHW (the forward API)
  kTailStep = 1,       // the ancestral update of x in place
  kTailX0 = 2,         // x0_out = clip(a0 x - b0 eps), x read only
  kTailX0Step = 3,     // the x0-form update of x in place (rows of xrow)
  kTailSse = 4,        // the denoising-error sums
  kTailX0StepMom = 5,  // kTailX0Step plus the x0 moments of every image
  kTailX0Step2M = 6,     // the second-order multistep x0-form update (the previous row's x0 from TailArgs::hist)
  kTailX0Step2MMom = 7,  // kTailX0Step2M plus the x0 moments of every image
};
// EPI, the tail kernels' template parameter: eps and step share instantiation 0 (a.step_mode tells them apart at
// run time); every other mode has its own. The four x0-form step modes have a second one each, EPI 7..10 (3, 5, 6, 7
// in this order): the same mode guided from the device tables gw_rows / gw_img (TailArgs::cfg == 2,
// itsd_set_guidance). They are instantiations of their own so that every other one keeps its code.
constexpr int kTailEpiGw = 7;  // the first table-guided instantiation
constexpr int kTailEpis = 11;
constexpr bool tail_epi_gw(int epi) { return epi >= kTailEpiGw; }
constexpr int tail_epi_base(int epi) { return epi < kTailEpiGw ? epi : epi == kTailEpiGw ? 2 : epi - 4; }
constexpr int tail_epi(int mode, bool gw = false) {
  return mode <= kTailStep ? 0 : !gw ? mode - 1 : mode == 3 ? kTailEpiGw : mode + 3;  // (gw: x0-form modes only)
}
// ... and back: the one mode of instantiation epi >= 1, eps or step for 0
constexpr TailMode tail_epi_mode(int epi, bool step) {
  return epi ? TailMode(tail_epi_base(epi) + 1) : step ? kTailStep : kTailEps;
}
// what a mode does
constexpr bool tail_reads_x(int mode) { return mode != kTailEps && mode != kTailSse; }
constexpr bool tail_loads_row(int mode) {  // row *tsel of the schedule tables and the run's parameters
  return mode == kTailStep || mode == kTailX0Step || mode == kTailX0StepMom || mode == kTailX0Step2M ||
         mode == kTailX0Step2MMom;
}
constexpr bool tail_x0_form(int mode) {
  return mode == kTailX0Step || mode == kTailX0StepMom || mode == kTailX0Step2M || mode == kTailX0Step2MMom;
}
constexpr bool tail_2m(int mode) { return mode == kTailX0Step2M || mode == kTailX0Step2MMom; }  // reads cp and hist
constexpr bool tail_traced(int mode) { return mode == kTailX0StepMom || mode == kTailX0Step2MMom; }
// the block statistics it ends in (tail_block_stats: 2 sums; 2 sums, min, max), 0 where it ends in none
constexpr int tail_stats(int mode) { return mode == kTailSse ? 2 : tail_traced(mode) ? 4 : 0; }
static_assert(tail_epi(kTailX0Step, true) == 7 && tail_epi(kTailX0StepMom, true) == 8 &&
                  tail_epi(kTailX0Step2M, true) == 9 && tail_epi(kTailX0Step2MMom, true) == 10 &&
                  tail_epi_mode(7, false) == kTailX0Step && tail_epi_mode(8, false) == kTailX0StepMom &&
                  tail_epi_mode(9, false) == kTailX0Step2M && tail_epi_mode(10, false) == kTailX0Step2MMom &&
                  tail_epi_mode(6, false) == kTailX0Step2MMom && tail_epi_mode(1, false) == kTailX0,
              "the table-guided instantiations and their modes");

struct TailArgs {
  const void* g;        // NHWC [nb][H][W][C] : silu(gn(h))
  const float* w;       // [3][C][3][3] fp32 (reference layout)
  const float* b;       // [3]
  int H, W, C, n;       // n = output images
  int cfg;              // eps = (1+w) eps(img) - w eps(img+n)  (DiffusionCondition.py:85): 1 w = guide_w; 2 (the x0-form
                        // step modes only) w = gw_rows[*tsel] (* gw_img[img]), below
  float guide_w;        // w (fp32 cast of the Python float)
  float guide_w1;       // (1 + w) computed in double then cast, as the reference's scalar
  // mode
  int step_mode;        // a TailMode (an int: the argument block's layout is fixed, below)
  float* eps_out;       // NCHW [n][3][H][W]
  float* x;             // NCHW [n][3][H][W]
  const int* tsel;      // current step t (device)
  // (the ancestral tables; the x0-form modes never read them, and the 2M modes keep their two operands in the storage
  // of the first two: xcp, the sixth row table cp[K], and hist, the previous row's x0 NCHW fp32 [n][3][H][W])
  union { const float* coeff1; const float* xcp; };
  union { const float* coeff2; float* hist; };
  // (cfg == 2: gw_rows, the guidance weight of every row, device fp32 [T_sched], in the storage of the third ancestral
  // table; and gw_img, the candidates' multipliers, device fp32 [n] or null = 1, in that of kTailX0's output)
  union { const float* sqrt_var; const float* gw_rows; };
  const float* noise;   // [T][n][3][H][W] or null
  const RunParams* run; // seed / noise offset / clip step of this run (device)
  int* nan_flag;
  // bf16 MFMA tail (tail_mfma_kernel): g is the RAW last ResBlock output and the tail
  // GroupNorm+SiLU is applied while staging it, with per-image coefficients
  // coef[img][C/8][a0..a7, b0..b7] (gn_coef_kernel); wmf = bf16 weights [9C/32][4][3][8]
  // (k = tap*C + ci; k-step ks, lane group kg, output channel, 8 consecutive k)
  const float* coef;
  const bf16_t* wmf;
  // kTailX0 (itsd_sampler_predict_x0): a0 = 1/sqrt(abar_t), b0 = sqrt(1/abar_t - 1) as fp32, output NCHW [n][3][H][W]
  float a0, b0;
  union { float* x0_out; const float* gw_img; };
  // kTailX0Step (itsd_sampler_run under an x0-form schedule, itsd_set_schedule_x0): row k = *tsel of five device
  // tables [K] -- a0, b0, c0, cx, sg in this order -- and whether the x_0 estimate is clipped. tsel, noise (indexed by
  // row), run and nan_flag as in kTailStep; coeff1 / coeff2 / sqrt_var are not read
  const float* xrow[5];
  int clip_x0;
  // kTailSse (itsd_verify_denoise): the denoising-error probe. Nothing is guided and nothing of the step's is read:
  // z[e] = noise[e] (here ONE field [3][H][W], shared by every image) or Philox (vseed, vstream, e), e the element
  // within the image; each block stores its (sum (z - eps_c)^2, sum (z - eps_u)^2) as one fp32 pair at
  // vpart[blockIdx.x] (blocks are image-major and never straddle two images) and tail_stats_finalize_kernel sums each
  // image's pairs in block order in fp64 into vsse[n][2]. eps_out, when non-null, receives the unguided
  // eps [1 or 2][n][3][H][W] (cond, then uncond). x is not read.
  // kTailX0StepMom (itsd_sampler_run with a score trace attached, itsd_sampler_set_trace): kTailX0Step on x, bit for
  // bit, and each block stores (sum x0, sum x0^2, min x0, max x0) of its output elements -- x0 the value the step used,
  // clipped iff clip_x0 -- as four fp32 at tpart[blockIdx.x] (blocks are image-major and never straddle two images);
  // tail_stats_finalize_kernel folds each image's blocks in block order in fp64 into
  // trace[(*tsel * trace_stride + img) * 4 + 0..3], for a row *tsel in [0, trace_rows).
  // Its operands share the storage of kTailSse's, which it never reads (and the reverse), and trace_stride sits in
  // what was padding: the struct keeps its size and offsets. The struct is the kernels' argument block, and a larger
  // one changed the register allocation of the existing tail_mfma_kernel instantiations.
  unsigned long long vseed;
  union { unsigned vstream; int trace_rows; };
  int trace_stride;
  union { float* vpart; float* tpart; };
  union { double* vsse; double* trace; };
  // kTailX0Step2M / kTailX0Step2MMom (itsd_sampler_run under itsd_set_schedule_x0_2m): the x0 step with the multistep
  // correction  m = ((c0*x0) + (cp*x0p)) + (cx*x),  cp = xcp[*tsel], x0p = hist[o] (this row's own x0 where
  // *tsel == RunParams::restart_at); a row with cp == 0 is kTailX0Step's expression and does not read hist. Every
  // row stores its x0 to hist[o]. The Mom form adds this row's x0 (not the combination) to the moments.
  // cfg == 2 (itsd_sampler_run with a guidance table attached, itsd_set_guidance; the four x0-form step modes, in
  // instantiations of their own):  w = gw_rows[*tsel] ; if (gw_img) w = w * gw_img[img] ; w1 = 1.0f + w ;
  // e = w1 * ec - w * eu  (fp32, no contraction: cfg == 1's expression and, for w == guide_w, its bits). img is the
  // candidate, never img + n; a block lies in one image, so w sits in scalar registers.
};
static_assert(sizeof(TailArgs) == 240, "TailArgs is the tail kernels' argument block: a larger one changed the "
                                       "register allocation of the existing instantiations (DESIGN section 13)");
static_assert(offsetof(TailArgs, xcp) == offsetof(TailArgs, coeff1) && offsetof(TailArgs, coeff1) == 80 &&
                  offsetof(TailArgs, hist) == offsetof(TailArgs, coeff2) && offsetof(TailArgs, coeff2) == 88 &&
                  offsetof(TailArgs, sqrt_var) == 96 && offsetof(TailArgs, gw_rows) == 96 &&
                  offsetof(TailArgs, gw_img) == offsetof(TailArgs, x0_out),
              "the 2M and guidance-table operands overlay the ancestral tables and kTailX0's output");

constexpr int kBranchChunk = 256;  // parent-table rows a branch_kernel launch carries in its arguments (1 KiB)

// The antithetic ES gradient (itsd_es_step): pairs a slice of es_grad_kernel sums, in ascending order, before
// es_adam_kernel adds the slices in slice order. It defines the summation order of the gradient (include/itsd.h names
// it), and so the rounding bound the tests assert. kEsItems: elements a thread of es_adam_kernel updates, so a block
// covers 256 * kEsItems elements and stores one fp64 partial of |g|^2.
constexpr int kEsSlice = 16;
constexpr int kEsItems = 4;
constexpr int kEsMaxPairs = kEsSlice * 65535;  // slices ride on gridDim.y
struct EsAdam { float beta1, omb1, beta2, omb2, c1, c2, eps; };  // itsd_adam_step (include/itsd.h), field for field

}  // namespace itsd
