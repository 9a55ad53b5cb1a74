// small_kernels.hip - the memory-bound / tiny kernels of the path (gfx950):
//   stem and head convolutions (NCHW <-> NHWC at the ABI edge, unet.py:78-80,145-149),
//   timestep embedding MLP (unet.py:63-68,151-169), batched mat-vec (ResBlock emb_layers
//   unet.py:286-289; n_cond==1 cross-attention collapse unet_attention.py:186-212),
//   note durations of a generated roll (pf_prmat2c_durations) and its integer statistics against the run's chords (pf_roll_stats),
//   the first-stage autoencoder's tail and front and the two posterior samplers, the clock and matrix-pipe probes,
//   GRU gate update and the texture-encoder front end (dl_modules/chord_enc.py:15-22, txt_enc.py:23-27).
// (The sampler's elementwise family - guidance, windows, updates, noise, inversion, slerp - is sampler_steps.hip.)
#include "elementwise.h"

namespace pf {

int num_cus() {
  static std::atomic<int> cache[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  int v = cache[dev & 63].load(std::memory_order_relaxed);
  if (v == 0) {
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    cache[dev & 63].store(v, std::memory_order_relaxed);
  }
  return v;
}

__device__ __forceinline__ float silu_s(float v) { return v / (1.0f + __expf(-v)); }

// ------------------------------------------------------------------ stem conv (Cin tiny)
// thread = (pixel, 4 output channels); x NCHW, out NHWC. Weights [Cout][Cin][3][3] read through LDS.
__global__ __launch_bounds__(256) void conv_in_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bias, float* __restrict__ out, int B, int Cin,
                                                      int Cout, int H, int W) {
  extern __shared__ float sw[];  // [Cout][Cin*9]
  const int K = Cin * 9;
  for (int i = threadIdx.x; i < Cout * K; i += 256) sw[i] = w[i];
  __syncthreads();
  const int CQ = Cout / 4;
  const size_t total = (size_t)B * H * W * CQ;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int cq = (int)(idx % CQ);
    const size_t pix = idx / CQ;
    const int xw = (int)(pix % W), yh = (int)((pix / W) % H), b = (int)(pix / ((size_t)W * H));
    float acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = bias[cq * 4 + j];
    for (int ci = 0; ci < Cin; ++ci) {
      const float* xp = x + ((size_t)b * Cin + ci) * H * W;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const int iy = yh + r - 1;
        if (iy < 0 || iy >= H) continue;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const int ix = xw + s - 1;
          if (ix < 0 || ix >= W) continue;
          const float v = xp[(size_t)iy * W + ix];
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j] = fmaf(v, sw[(cq * 4 + j) * K + ci * 9 + r * 3 + s], acc[j]);
        }
      }
    }
    *reinterpret_cast<float4*>(out + pix * Cout + cq * 4) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  }
}

// Register-weight variant: a workgroup owns a 16x16 pixel tile, stages its 18x18xCIN input halo in LDS once, and every
// thread keeps the 4 x CIN x 9 weights of ONE output-channel quad in registers while it walks the 16 pixels of a tile
// column.  A pixel's Cout floats are written by 16 adjacent lanes as one contiguous NHWC run (16 bytes per lane).
template <int CIN>
__global__ __launch_bounds__(256) void conv_in_reg_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ out, int B,
                                                          int H, int W, float* __restrict__ stats) {
  constexpr int K = CIN * 9, T = 16, TI = T + 2, COUT = 64;
  __shared__ float sx[CIN][TI][TI + 1];
  __shared__ float sred[16][16][8];   // [pixel column][channel quad][4 sums | 4 sums of squares] (statistics only)
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  const int tilesx = (W + T - 1) / T, tilesy = (H + T - 1) / T;
  const int tx = bid % tilesx; bid /= tilesx;
  const int ty = bid % tilesy;
  const int b = bid / tilesy;
  for (int u = tid; u < CIN * TI * TI; u += 256) {
    const int ci = u / (TI * TI), r = (u / TI) % TI, c = u % TI;
    const int iy = ty * T + r - 1, ix = tx * T + c - 1;
    sx[ci][r][c] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? x[((size_t)b * CIN + ci) * H * W + (size_t)iy * W + ix] : 0.f;
  }
  const int cq = tid & 15, px = tid >> 4;
  float wr[4][K], bj[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bj[j] = bias[cq * 4 + j];
#pragma unroll
    for (int k = 0; k < K; ++k) wr[j][k] = w[(size_t)(cq * 4 + j) * K + k];
  }
  __syncthreads();
  const int ox = tx * T + px;
  float ssum[4] = {0.f, 0.f, 0.f, 0.f}, ssq[4] = {0.f, 0.f, 0.f, 0.f};
  if (ox < W) {
#pragma unroll 4
  for (int py = 0; py < T; ++py) {
    const int oy = ty * T + py;
    if (oy >= H) break;
    float acc[4] = {bj[0], bj[1], bj[2], bj[3]};
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int s2 = 0; s2 < 3; ++s2) {
          const float v = sx[ci][py + r][px + s2];
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j] = fmaf(v, wr[j][ci * 9 + r * 3 + s2], acc[j]);   // order: ci, then tap
        }
    *reinterpret_cast<float4*>(out + (((size_t)b * H + oy) * W + ox) * COUT + cq * 4) = make_float4(acc[0], acc[1], acc[2], acc[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j) { ssum[j] += acc[j]; ssq[j] += acc[j] * acc[j]; }
  }
  }
  // per-tile channel (sum, sumsq) of what was stored, in the layout of the conv epilogues' statistics ([B][tiles][64][2]): the
  // GroupNorm of the first ResBlock then needs no pass over the stem output (deterministic: fixed reduction order)
  if (stats) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { sred[px][cq][j] = ssum[j]; sred[px][cq][4 + j] = ssq[j]; }
    __syncthreads();
    if (tid < COUT) {
      const int q = tid >> 2, j = tid & 3;
      float a = 0.f, qq = 0.f;
#pragma unroll
      for (int c = 0; c < 16; ++c) { a += sred[c][q][j]; qq += sred[c][q][4 + j]; }
      float* dst = stats + (((size_t)b * (tilesx * tilesy) + ty * tilesx + tx) * COUT + tid) * 2;
      dst[0] = a; dst[1] = qq;
    }
  }
}

int launch_conv_in_stats_tiles(int cin, int cout, int h, int w_) { return (cin <= 2 && cout == 64) ? cdiv(h, 16) * cdiv(w_, 16) : 0; }

int launch_conv_in(const float* x, const float* w, const float* bias, float* out, int batch, int cin, int cout, int h, int w_,
                   hipStream_t stream, float* stats) {
  PF_REQUIRE(!stats || launch_conv_in_stats_tiles(cin, cout, h, w_) > 0, "conv_in: statistics only from the register-weight kernel (cin <= 2, cout == 64)");
  PF_REQUIRE(cout % 4 == 0 && (size_t)cout * cin * 9 * 4 <= 64 * 1024, "conv_in: unsupported channel counts %d->%d", cin, cout);
  const size_t total = (size_t)batch * h * w_ * (cout / 4);
  if (cin <= 2 && cout == 64) {
    const int grid = batch * cdiv(h, 16) * cdiv(w_, 16);
    if (cin == 1) hipLaunchKernelGGL(conv_in_reg_kernel<1>, dim3(grid), dim3(256), 0, stream, x, w, bias, out, batch, h, w_, stats);
    else hipLaunchKernelGGL(conv_in_reg_kernel<2>, dim3(grid), dim3(256), 0, stream, x, w, bias, out, batch, h, w_, stats);
    PF_CHECK_HIP(hipGetLastError());
    return PF_OK;
  }
  const int grid = (int)min((size_t)4096, (total + 255) / 256);
  hipLaunchKernelGGL(conv_in_kernel, dim3(grid), dim3(256), (size_t)cout * cin * 9 * sizeof(float), stream, x, w, bias, out, batch,
                     cin, cout, h, w_);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}

// ------------------------------------------------------------------ head: GN+SiLU -> conv3x3 -> few channels, NCHW out
// HBM-bound by construction (B x H x W x Cin floats in, a few channels out: 67 MB at the bench shape, 0.6 GFLOP), so the job is to keep the
// memory pipe busy: 16x16 output pixels per block, the normalised + activated 18x18 halo staged in LDS 16 channels at a time, and
//   * the NEXT chunk's global loads are issued (into registers) before the current chunk's arithmetic, so every block overlaps its own
//     memory latency instead of leaving that to its neighbours on the CU;
//   * SiLU with the hardware reciprocal (silu_f of conv_common.h) - an IEEE division per element costs as much as the rest of the transform;
//   * weights packed [9][Cin][Cout]: a tap's Cout weights of one input channel are adjacent, wave-uniform addresses -> scalar loads, and for
//     two / four output channels one v_pk_fma_f32 feeds two accumulators (half the VALU instructions of the dot products).
typedef float f32x2_s __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float silu_fast(float v) { return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }

template <int COUT>
__global__ __launch_bounds__(256) void conv_out_kernel(const float* __restrict__ x, const float* __restrict__ sc,
                                                       const float* __restrict__ sh, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ out, int B, int Cin,
                                                       int H, int W) {
  constexpr int T = 16, TI = T + 2, CK = 16, CP = CK + 4, NPIECE = TI * TI * (CK / 4), NP = (NPIECE + 255) / 256;
  constexpr int NPAIR = COUT / 2, ODD = COUT & 1;
  __shared__ __attribute__((aligned(16))) float sx[TI * TI * CP];
  const int tid = threadIdx.x;
  const int tilesx = (W + T - 1) / T, tilesy = (H + T - 1) / T;
  int bid = blockIdx.x;
  const int tx = bid % tilesx; bid /= tilesx;
  const int ty = bid % tilesy;
  const int b = bid / tilesy;
  const int py = tid / T, px = tid % T;
  // this thread's pieces of a chunk (a piece = four channels of one halo pixel): fixed across the chunks.  256 % 4 == 0, so the
  // channel quad (tid & 3) - and with it the thread's scale / shift vectors - is the same for all of them.
  const int c4 = tid & 3;
  // Loads are unconditional (padding / surplus pieces read the tile's first valid element and are zeroed by a select when staged):
  // no exec-mask branches between them, all NP loads of a chunk in flight together.
  unsigned goff[NP];
  int soff[NP];
  float keep[NP];                          // 1: a pixel inside the image, 0: conv padding (zeros of the ACTIVATED tensor)
  const unsigned gsafe = (unsigned)(((b * H + min(ty * T, H - 1)) * W + min(tx * T, W - 1)) * Cin) + c4 * 4;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int u = tid + i * 256, pix = u >> 2;
    const int iy = ty * T + pix / TI - 1, ix = tx * T + pix % TI - 1;
    const bool in = u < NPIECE && iy >= 0 && iy < H && ix >= 0 && ix < W;
    soff[i] = u < NPIECE ? pix * CP + c4 * 4 : -1;
    goff[i] = in ? (unsigned)(((b * H + iy) * W + ix) * Cin) + c4 * 4 : gsafe;
    keep[i] = in ? 1.f : 0.f;
  }
  f32x4 r[NP], a4, d4;
  auto load = [&](int c0) {
#pragma unroll
    for (int i = 0; i < NP; ++i) r[i] = *reinterpret_cast<const f32x4*>(x + (size_t)goff[i] + c0);
    a4 = *reinterpret_cast<const f32x4*>(sc + (size_t)b * Cin + c0 + c4 * 4);
    d4 = *reinterpret_cast<const f32x4*>(sh + (size_t)b * Cin + c0 + c4 * 4);
  };
  auto stage = [&]() {   // normalise + SiLU
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      f32x4 v = r[i] * a4 + d4;
      v[0] = silu_fast(v[0]) * keep[i]; v[1] = silu_fast(v[1]) * keep[i]; v[2] = silu_fast(v[2]) * keep[i]; v[3] = silu_fast(v[3]) * keep[i];
      if (soff[i] >= 0) *reinterpret_cast<f32x4*>(sx + soff[i]) = v;
    }
  };
  f32x2_s acc2[NPAIR > 0 ? NPAIR : 1];
  float acc1 = 0.f;
#pragma unroll
  for (int q = 0; q < NPAIR; ++q) acc2[q] = f32x2_s{0.f, 0.f};
  load(0);
  stage();
  __syncthreads();
  for (int c0 = 0; c0 < Cin; c0 += CK) {
    const bool more = c0 + CK < Cin;
    if (more) load(c0 + CK);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const float* xp = sx + ((py + t / 3) * TI + px + t % 3) * CP;
      const float* wt = w + (size_t)__builtin_amdgcn_readfirstlane((t * Cin + c0) * COUT);   // [tap][Cin][COUT]: uniform address -> scalar loads
#pragma unroll
      for (int k4 = 0; k4 < CK / 4; ++k4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xp + k4 * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float* we = wt + (k4 * 4 + e) * COUT;
#pragma unroll
          for (int q = 0; q < NPAIR; ++q)
            acc2[q] = __builtin_elementwise_fma(f32x2_s{v[e], v[e]}, f32x2_s{we[2 * q], we[2 * q + 1]}, acc2[q]);
          if (ODD) acc1 = fmaf(v[e], we[COUT - 1], acc1);
        }
      }
    }
    __syncthreads();            // every thread has finished reading this chunk's image
    if (more) {
      stage();
      __syncthreads();
    }
  }
  const int oy = ty * T + py, ox = tx * T + px;
  if (oy < H && ox < W) {
#pragma unroll
    for (int co = 0; co < COUT; ++co) {
      const float a = (ODD && co == COUT - 1) ? acc1 : acc2[co / 2][co & 1];
      out[(((size_t)b * COUT + co) * H + oy) * W + ox] = a + bias[co];
    }
  }
}

int launch_conv_out(const float* x, const float* sc, const float* sh, const float* w, const float* bias, float* out, int batch,
                    int cin, int cout, int h, int w_, hipStream_t stream) {
  PF_REQUIRE(cout >= 1 && cout <= 4 && cin % 16 == 0, "conv_out: unsupported channel counts %d->%d", cin, cout);
  PF_REQUIRE((size_t)batch * h * w_ * cin < ((size_t)1 << 31), "conv_out: tensor too large for 32-bit element offsets");
  const int grid = batch * cdiv(h, 16) * cdiv(w_, 16);
  switch (cout) {
    case 1: hipLaunchKernelGGL(conv_out_kernel<1>, dim3(grid), dim3(256), 0, stream, x, sc, sh, w, bias, out, batch, cin, h, w_); break;
    case 2: hipLaunchKernelGGL(conv_out_kernel<2>, dim3(grid), dim3(256), 0, stream, x, sc, sh, w, bias, out, batch, cin, h, w_); break;
    case 3: hipLaunchKernelGGL(conv_out_kernel<3>, dim3(grid), dim3(256), 0, stream, x, sc, sh, w, bias, out, batch, cin, h, w_); break;
    default: hipLaunchKernelGGL(conv_out_kernel<4>, dim3(grid), dim3(256), 0, stream, x, sc, sh, w, bias, out, batch, cin, h, w_); break;
  }
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}

// ------------------------------------------------------------------ output step: onset/sustain image -> note durations
// utils.py:240-269 / 433-476 of the reference: a note starts where round(onset) > 0 and lasts while round(sustain) > 0 on
// the following steps of the same key.  Python's round is half-to-even on these float32 values, so the predicate is
// exactly v > 0.5 (custom_round: 0.95 < v < 1.05, onset only).  One thread per (image, key) column walks its S steps
// backwards keeping the length of the sustain run that starts at the next step: a single coalesced pass over the image
// (lanes = consecutive keys), 4 B read per input element, 4 B written per output element.
__global__ __launch_bounds__(128) void prmat2c_durations_kernel(const float* __restrict__ x, int S, int custom_round,
                                                                int32_t* __restrict__ dur) {
  const int n = blockIdx.x, key = threadIdx.x;
  const float* on = x + ((size_t)n * 2 + 0) * S * 128 + key;
  const float* su = x + ((size_t)n * 2 + 1) * S * 128 + key;
  int32_t* d = dur + (size_t)n * S * 128 + key;
  int run = 0;                                   // sustain run starting at step t+1
  for (int t = S - 1; t >= 0; --t) {
    const float o = on[(size_t)t * 128], sv = su[(size_t)t * 128];
    const bool is_on = custom_round ? (o > 0.95f && o < 1.05f) : (o > 0.5f);
    d[(size_t)t * 128] = is_on ? 1 + run : 0;
    run = (sv > 0.5f) ? run + 1 : 0;
  }
}

int launch_prmat2c_durations(const float* x, int n, int steps, int custom_round, int32_t* dur, hipStream_t stream) {
  PF_REQUIRE(x && dur && n > 0 && steps > 0, "prmat2c_durations: bad arguments");
  hipLaunchKernelGGL(prmat2c_durations_kernel, dim3(n), dim3(128), 0, stream, x, steps, custom_round, dur);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}

// ------------------------------------------------------------------ roll statistics: onset/sustain image (+ chords, + mask) -> integers
// include/pfhip.h, pf_roll_stats; DESIGN.md 3, "Roll statistics".  One workgroup per image, one wave per beat at a time: lane l of a wave is
// key l, then key 64 + l, of each of the beat's four steps (a 256-byte coalesced read per channel and half), and a __ballot turns the
// wave's 64 predicates into one word.  Everything a beat contributes is then popcounts and bit tests of those words - wave-uniform
// integers - except the per-class counts, which lane k < 12 keeps for class k as popcount(word & class_mask[k]): the keys of class k
// among the lower 64 are bits k, k + 12, ..., and among the upper 64 (key = 64 + bit, 64 % 12 == 4) the bits of class (k + 8) % 12.
// A beat is owned by one wave, so its rows of `chroma` and `onsets` are written without any combination; the image's counters are added
// over the waves through a few LDS integers.  No atomics, no floating-point arithmetic at all: exact and order-free.
constexpr int kRollMaxWaves = 16;
__device__ __forceinline__ bool roll_round(float v, int custom) { return custom ? (v > 0.95f && v < 1.05f) : (v > 0.5f); }
__device__ __forceinline__ bool roll_occupied(float v, int custom) { return custom ? (v > 0.95f && v < 1.05f) : (v > 0.5f || v < -0.5f); }
// arg-max of twelve floats, ties (and a NaN, which never compares greater) to the lowest index; *any: some entry is > 0
__device__ __forceinline__ int roll_argmax12(const float* __restrict__ v, bool* any) {
  float best = v[0];
  int bi = 0;
  bool pos = best > 0.0f;
  for (int i = 1; i < 12; ++i) {
    const float c = v[i];
    pos = pos || c > 0.0f;
    if (c > best) { best = c; bi = i; }
  }
  *any = pos;
  return bi;
}

__global__ __launch_bounds__(64 * kRollMaxWaves) void roll_stats_kernel(const float* __restrict__ x, const float* __restrict__ chord,
                                                                        const float* __restrict__ mask, int steps, int custom, int bass_rel,
                                                                        int32_t* __restrict__ counters, int32_t* __restrict__ chroma,
                                                                        int32_t* __restrict__ onsets) {
  __shared__ int32_t part[kRollMaxWaves][PF_ROLL_NCOUNT];
  const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6, beats = steps >> 2;
  const float* on = x + (size_t)n * 2 * steps * 128;
  const float* su = on + (size_t)steps * 128;
  const float* mk = mask ? mask + (size_t)n * 2 * steps * 128 : nullptr;
  constexpr unsigned long long kClass0 = 0x1001001001001001ull;                 // keys 0, 12, ..., 60
  const unsigned long long cm[2] = {lane < 12 ? kClass0 << lane : 0ull, lane < 12 ? kClass0 << ((lane + 8) % 12) : 0ull};
  const int cls[2] = {lane % 12, (lane + 4) % 12};                              // class of this lane's key in the lower / upper half
  int cnt[PF_ROLL_NCOUNT] = {0};
  int low = 128, high = -1;
  for (int j = wave; j < beats; j += nwaves) {
    // the beat's chord: the class set as 12 bits, the same set as key bits of the two halves, the bass class (-1: none)
    unsigned cset = 0;
    int bass = -1;
    if (chord) {
      const float* cd = chord + ((size_t)n * beats + j) * 36;
      cset = (unsigned)__ballot(lane < 12 && cd[12 + (lane < 12 ? lane : 0)] > 0.5f);
      bool any;
      int b = roll_argmax12(cd + 24, &any);
      if (bass_rel) {
        bool unused;
        b = (b + roll_argmax12(cd, &unused)) % 12;
      }
      bass = any ? b : -1;
    }
    const unsigned long long cw[2] = {__ballot((cset >> cls[0]) & 1u), __ballot((cset >> cls[1]) & 1u)};
    // every value of the beat first (the loads are independent), then the words
    const int t0 = 4 * j;
    float a[4][2], s[4][2], m[4][2], pa[2], ps[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const size_t p = (size_t)(t0 > 0 ? t0 - 1 : 0) * 128 + 64 * h + lane;
      pa[h] = t0 > 0 ? on[p] : 0.0f;                                            // 0 is unoccupied under both rules
      ps[h] = t0 > 0 ? su[p] : 0.0f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const size_t i = (size_t)(t0 + k) * 128 + 64 * h + lane;
        a[k][h] = on[i];
        s[k][h] = su[i];
        m[k][h] = mk ? mk[i] : 0.0f;
      }
    }
    int mine = 0, snd_beat = 0, on_beat = 0, snd_in = 0, on_in = 0, orphan = 0;
    unsigned long long heard[2] = {0ull, 0ull};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int on_step = 0;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const bool live = m[k][h] == 0.0f;
        const bool is_on = live && roll_round(a[k][h], custom), is_su = live && roll_round(s[k][h], custom);
        const bool occ = roll_occupied(pa[h], custom) || roll_occupied(ps[h], custom);
        const unsigned long long w_on = __ballot(is_on), w_snd = __ballot(is_on || is_su), w_orph = __ballot(is_su && !occ);
        pa[h] = a[k][h];
        ps[h] = s[k][h];
        on_step += __popcll(w_on);
        snd_beat += __popcll(w_snd);
        snd_in += __popcll(w_snd & cw[h]);
        on_in += __popcll(w_on & cw[h]);
        orphan += __popcll(w_orph);
        mine += __popcll(w_snd & cm[h]);
        heard[h] |= w_snd;
      }
      on_beat += on_step;
      if (lane == 0) onsets[(size_t)n * steps + t0 + k] = on_step;
    }
    if (lane < 12) chroma[((size_t)n * beats + j) * 12 + lane] = mine;
    const int n_heard = __popcll(__ballot(lane < 12 && ((cset >> (lane & 15)) & 1u) && mine > 0));
    cnt[PF_ROLL_N_ONSET] += on_beat;
    cnt[PF_ROLL_N_SOUNDING] += snd_beat;
    cnt[PF_ROLL_N_ORPHAN] += orphan;
    const bool sounds = (heard[0] | heard[1]) != 0ull;
    const int lowest = heard[0] ? __builtin_ctzll(heard[0]) : heard[1] ? 64 + __builtin_ctzll(heard[1]) : 128;
    const int highest = heard[1] ? 127 - __builtin_clzll(heard[1]) : heard[0] ? 63 - __builtin_clzll(heard[0]) : -1;
    low = min(low, lowest);
    high = max(high, highest);
    if (cset) {
      cnt[PF_ROLL_CHORD_BEATS] += 1;
      cnt[PF_ROLL_SOUND_ON_CHORD] += snd_beat;
      cnt[PF_ROLL_SOUND_IN_CHORD] += snd_in;
      cnt[PF_ROLL_ONSET_IN_CHORD] += on_in;
      cnt[PF_ROLL_ONSET_ON_CHORD] += on_beat;
      cnt[PF_ROLL_CHORD_CLASSES] += __popc(cset);
      cnt[PF_ROLL_CHORD_HEARD] += n_heard;
      if (bass >= 0 && sounds) {
        cnt[PF_ROLL_BASS_BEATS] += 1;
        cnt[PF_ROLL_BASS_HIT] += (lowest % 12 == bass) ? 1 : 0;
      }
    }
  }
  cnt[PF_ROLL_LOW_KEY] = low;
  cnt[PF_ROLL_HIGH_KEY] = high;
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < PF_ROLL_NCOUNT; ++c) part[wave][c] = cnt[c];
  }
  __syncthreads();
  if (threadIdx.x < PF_ROLL_NCOUNT) {
    const int c = threadIdx.x;
    int v = part[0][c];
    for (int w = 1; w < nwaves; ++w) v = c == PF_ROLL_LOW_KEY ? min(v, part[w][c]) : c == PF_ROLL_HIGH_KEY ? max(v, part[w][c]) : v + part[w][c];
    if (c == PF_ROLL_LOW_KEY && v == 128) v = -1;
    counters[(size_t)n * PF_ROLL_NCOUNT + c] = v;
  }
}

int launch_roll_stats(const pf_roll_stats_args& a, hipStream_t stream) {
  PF_REQUIRE(a.prmat2c && a.n > 0 && a.steps > 0, "roll_stats: bad arguments (prmat2c %p, n = %d, steps = %d)", (const void*)a.prmat2c, a.n, a.steps);
  PF_REQUIRE(a.steps % 4 == 0, "roll_stats: steps = %d is not a whole number of beats (4 steps each)", a.steps);
  PF_REQUIRE(a.counters && a.chroma && a.onsets, "roll_stats: null output (counters %p, chroma %p, onsets %p)", (void*)a.counters, (void*)a.chroma,
             (void*)a.onsets);
  const uintptr_t all = (uintptr_t)a.prmat2c | (uintptr_t)a.chord | (uintptr_t)a.mask | (uintptr_t)a.counters | (uintptr_t)a.chroma | (uintptr_t)a.onsets;
  PF_REQUIRE(all % 4 == 0, "roll_stats: every pointer must be 4-byte aligned");
  const int waves = min(kRollMaxWaves, a.steps / 4);
  hipLaunchKernelGGL(roll_stats_kernel, dim3(a.n), dim3(64 * waves), 0, stream, a.prmat2c, a.chord, a.mask, a.steps, a.custom_round != 0,
                     a.bass_relative != 0, a.counters, a.chroma, a.onsets);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}

// ------------------------------------------------------------------ timestep embedding MLP
// out[b][:] = silu( W2 . silu(W0 . [cos(t f) | sin(t f)] + b0) + b2 )   (the SiLU of emb_layers is folded in)
__global__ __launch_bounds__(256) void time_embed_kernel(const int64_t* __restrict__ t, const float* __restrict__ w0,
                                                         const float* __restrict__ b0, const float* __restrict__ w2,
                                                         const float* __restrict__ b2, float* __restrict__ out, int channels,
                                                         int d_t) {
  extern __shared__ float sm[];  // e[channels] | h[d_t]
  float* e = sm;
  float* hbuf = sm + channels;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int half = channels / 2;
  const float tv = t ? (float)t[b] : (float)b;   // t == nullptr: the table form, row b = time-step value b
  for (int i = tid; i < 2 * half; i += 256) {
    const int j = i % half;
    float a = -9.210340371976184f * (float)j;  // -ln(10000) * j / half, evaluated in fp32 like the reference
    a = a / (float)half;
    const float arg = tv * expf(a);
    e[i] = (i < half) ? cosf(arg) : sinf(arg);
  }
  __syncthreads();
  for (int n = tid; n < d_t; n += 256) {
    float acc = b0[n];
    const float* wr = w0 + (size_t)n * channels;
    for (int k = 0; k < channels; ++k) acc = fmaf(wr[k], e[k], acc);
    hbuf[n] = silu_s(acc);
  }
  __syncthreads();
  for (int n = tid; n < d_t; n += 256) {
    float acc = b2[n];
    const float* wr = w2 + (size_t)n * d_t;
    for (int k = 0; k < d_t; ++k) acc = fmaf(wr[k], hbuf[k], acc);
    out[(size_t)b * d_t + n] = silu_s(acc);
  }
}

int launch_time_embed(const int64_t* t, const float* w0, const float* b0, const float* w2, const float* b2, float* out_silu,
                      int batch, int channels, int d_t, hipStream_t stream) {
  PF_REQUIRE(channels % 2 == 0 && channels + d_t <= 8192, "time_embed: unsupported sizes");
  hipLaunchKernelGGL(time_embed_kernel, dim3(batch), dim3(256), (size_t)(channels + d_t) * sizeof(float), stream, t, w0, b0, w2,
                     b2, out_silu, channels, d_t);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}

// ------------------------------------------------------------------ batched mat-vec: y[b][n] = W[n][:] . x[b][:] + bias[n]
// A wave owns 8 outputs x 8 K-slices (lane = 8*o + j): the 8 lanes of an output stride its weight row in 128-byte
// pieces, every lane keeps 8 batch-row accumulators, and the cross-lane reduction is 3 shuffles per accumulator.
// 8 batch rows per block, so a weight row is read once per 8 samples.  The block first stages its 8 input rows in LDS
// (the only data every output needs), so the global loads of the main loop are the weight pieces alone - independent,
// unrolled 8 deep, all in flight together - instead of nine dependent-latency loads per K step.
// Each row's accumulation is an explicit fmaf chain in a fixed order (identical for every row: batch-position invariant).
// EXP: the stored value is expf(y) (the scale head of the Polydis encoders, exp(linear_var(h))); the sums are the same.
template <bool EXP>
__global__ __launch_bounds__(256) void matvec_kernel(const float* __restrict__ x0, int ldx, const float* __restrict__ w,
                                                     const float* __restrict__ bias, float* __restrict__ y, int ldy, int B, int N,
                                                     int K, int n_per_group, int x_group_stride) {
  constexpr int RB = 8;
  extern __shared__ __attribute__((aligned(16))) float sx[];   // [RB][K] (vector path only)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int o = lane >> 3, j = lane & 7;
  const int b0 = blockIdx.y * RB;
  const int nb = min(RB, B - b0);
  const int n = (blockIdx.x * 4 + wave) * 8 + o;
  const int nc = min(n, N - 1);                                       // out-of-range outputs compute a duplicate, never store
  const float* wr = w + (size_t)nc * K;
  float acc[RB];
#pragma unroll
  for (int r = 0; r < RB; ++r) acc[r] = 0.f;
  const bool vec = (K % 32 == 0) && (ldx % 4 == 0) && (x_group_stride % 4 == 0);
  // the grouped (block-diagonal) form gives every output group its own input slice: stage only when the block shares one
  const int g_first = (blockIdx.x * 32) / n_per_group, g_last = (min(blockIdx.x * 32 + 31, N - 1)) / n_per_group;
  if (vec && g_first == g_last) {
    const float* xg = x0 + (size_t)g_first * x_group_stride;
    for (int i = threadIdx.x; i < RB * (K / 4); i += 256) {
      const int r = i / (K / 4), k4 = i % (K / 4);
      *reinterpret_cast<float4*>(sx + r * K + k4 * 4) = *reinterpret_cast<const float4*>(xg + (size_t)(b0 + min(r, nb - 1)) * ldx + k4 * 4);
    }
    __syncthreads();
    for (int kb = 0; kb < K; kb += 256) {
      float4 wv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k = kb + (j + 8 * u) * 4;
        wv[u] = k < K ? *reinterpret_cast<const float4*>(wr + k) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k = kb + (j + 8 * u) * 4;
        if (k < K) {
#pragma unroll
          for (int r = 0; r < RB; ++r) {
            const float4 xv = *reinterpret_cast<const float4*>(sx + r * K + k);
            acc[r] = fmaf(wv[u].w, xv.w, fmaf(wv[u].z, xv.z, fmaf(wv[u].y, xv.y, fmaf(wv[u].x, xv.x, acc[r]))));
          }
        }
      }
    }
  } else {
    const float* x = x0 + (size_t)(nc / n_per_group) * x_group_stride;
    for (int k = j; k < K; k += 8) {
      const float wv = wr[k];
#pragma unroll
      for (int r = 0; r < RB; ++r) acc[r] = fmaf(wv, x[(size_t)(b0 + min(r, nb - 1)) * ldx + k], acc[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    float v = acc[r];
    v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
    if (j == 0 && n < N && r < nb) {
      const float o = v + (bias ? bias[n] : 0.f);
      y[(size_t)(b0 + r) * ldy + n] = EXP ? expf(o) : o;
    }
  }
}

template <bool EXP>
static int launch_matvec_t(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int batch, int n, int k,
                           hipStream_t stream, int n_per_group, int x_group_stride) {
  PF_REQUIRE(x && w && y && batch > 0 && n > 0 && k > 0, "matvec: bad arguments");
  if (n_per_group <= 0) { n_per_group = n; x_group_stride = 0; }
  PF_REQUIRE((size_t)8 * k * sizeof(float) <= 64 * 1024, "matvec: K=%d too large for the staged input rows", k);
  hipLaunchKernelGGL(matvec_kernel<EXP>, dim3(cdiv(n, 32), cdiv(batch, 8)), dim3(256), (size_t)8 * k * sizeof(float), stream, x, ldx, w, bias, y, ldy,
                     batch, n, k, n_per_group, x_group_stride);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}
int launch_matvec(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int batch, int n, int k,
                  hipStream_t stream, int n_per_group, int x_group_stride) {
  return launch_matvec_t<false>(x, ldx, w, bias, y, ldy, batch, n, k, stream, n_per_group, x_group_stride);
}
int launch_matvec_exp(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int batch, int n, int k,
                      hipStream_t stream) {
  return launch_matvec_t<true>(x, ldx, w, bias, y, ldy, batch, n, k, stream, 0, 0);
}

// ------------------------------------------------------------------ first-stage autoencoder: posterior sample, encoder tail, decoder front
// GaussianDistribution.sample times the latent scaling factor (autoencoder.py:316-324, latent_diffusion.py:112-120).
// NOT inlined, contraction off: the encoder tail and gaussian_sample_body must give the same bits for the same moments and noise
// (see philox_normal4v).
__device__ __noinline__ float gaussian_sample1(float mean, float log_var, float nz, float scale) {
#pragma clang fp contract(off)
  const float sd = expf(0.5f * log_var);
  return scale * (mean + sd * nz);
}
// element i of a noise tensor, or - noise == nullptr - what randn_kernel(seed, sid, off) writes at i
__device__ __forceinline__ float noise_at(const float* __restrict__ noise, size_t i, uint64_t seed, uint64_t sid, uint64_t off) {
  if (noise) return noise[i];
  const uint64_t e = off + i;
  const f32x4 v = philox_normal4v(e >> 2, sid, seed);
  const int j = (int)(e & 3);
  return j == 0 ? v[0] : j == 1 ? v[1] : j == 2 ? v[2] : v[3];
}
struct gaussian_sample_body {
  const float* __restrict__ mean; const float* __restrict__ log_var; const float* __restrict__ noise; uint64_t seed, sid, off; float scale;
  float* __restrict__ z;
  __device__ __forceinline__ void begin() {}
  template <int V>
  __device__ __forceinline__ void at(size_t i) const { z[i] = gaussian_sample1(mean[i], log_var[i], noise_at(noise, i, seed, sid, off), scale); }
};
int launch_gaussian_sample(const float* mean, const float* log_var, const float* noise, uint64_t seed, uint64_t sid, uint64_t off, float scale,
                           float* z, size_t n, hipStream_t s) {
  PF_REQUIRE(mean && log_var && z && n > 0, "gaussian_sample: bad arguments");
  return ew_launch_v<1>(gaussian_sample_body{mean, log_var, noise, seed, sid, off, scale, z}, n, s);
}

// Normal(mean, std).rsample() (torch.distributions: loc + eps * scale as two rounded tensor operations); noise as above
struct normal_rsample_body {
  const float* __restrict__ mean; const float* __restrict__ sd; const float* __restrict__ noise; uint64_t seed, sid, off; float* __restrict__ z;
  __device__ __forceinline__ void begin() {}
  template <int V>
  __device__ __forceinline__ void at(size_t i) const { z[i] = add_rn(mean[i], mul_rn(noise_at(noise, i, seed, sid, off), sd[i])); }
};
int launch_normal_rsample(const float* mean, const float* sd, const float* noise, uint64_t seed, uint64_t sid, uint64_t off, float* z, size_t n,
                          hipStream_t s) {
  PF_REQUIRE(mean && sd && z && n > 0, "normal_rsample: bad arguments");
  return ew_launch_v<1>(normal_rsample_body{mean, sd, noise, seed, sid, off, z}, n, s);
}

// Encoder tail (autoencoder.py:198-201, 64-68, 316-324): moments = quant_conv(conv_out(swish(norm_out(x)))), mean | log_var = its halves,
// log_var clamped to [-30, 20], z = scale * (mean + exp(0.5 log_var) * noise); x NHWC, outputs NCHW.  The layout of conv_out_kernel: a
// workgroup owns 16x16 output pixels and stages the normalised + activated 18x18 halo in LDS 16 channels at a time; a thread owns one
// pixel and all Z2 = 2 z_channels outputs of the 3x3 conv, so the 1x1 quant_conv and everything behind it stay in its registers.
// Weights [9][Cin][Z2] at wave-uniform addresses (scalar loads).
template <int Z2>
__global__ __launch_bounds__(256) void ae_tail_kernel(const float* __restrict__ x, const float* __restrict__ sc, const float* __restrict__ sh,
                                                      const float* __restrict__ w, const float* __restrict__ bias, const float* __restrict__ qw,
                                                      const float* __restrict__ qb, int E2, const float* __restrict__ noise, uint64_t seed,
                                                      uint64_t sid, uint64_t off, float scale, float* __restrict__ z, float* __restrict__ mean,
                                                      float* __restrict__ log_var, int B, int Cin, int H, int W) {
  constexpr int T = 16, TI = T + 2, CK = 16, CP = CK + 4, NPIECE = TI * TI * (CK / 4);
  __shared__ __attribute__((aligned(16))) float sx[TI * TI * CP];
  const int tid = threadIdx.x;
  const int tilesx = (W + T - 1) / T, tilesy = (H + T - 1) / T;
  int bid = blockIdx.x;
  const int tx = bid % tilesx; bid /= tilesx;
  const int ty = bid % tilesy;
  const int b = bid / tilesy;
  const int py = tid / T, px = tid % T;
  float acc[Z2];
#pragma unroll
  for (int j = 0; j < Z2; ++j) acc[j] = 0.f;
  for (int c0 = 0; c0 < Cin; c0 += CK) {
    if (c0) __syncthreads();   // every thread has finished reading the previous chunk's image
    for (int u = tid; u < NPIECE; u += 256) {
      const int pix = u >> 2, c4 = u & 3;
      const int iy = ty * T + pix / TI - 1, ix = tx * T + pix % TI - 1;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};   // conv padding: zeros of the ACTIVATED tensor
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
        const f32x4 r = *reinterpret_cast<const f32x4*>(x + (((size_t)b * H + iy) * W + ix) * Cin + c0 + c4 * 4);
        const f32x4 a4 = *reinterpret_cast<const f32x4*>(sc + (size_t)b * Cin + c0 + c4 * 4);
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(sh + (size_t)b * Cin + c0 + c4 * 4);
        v = r * a4 + d4;
        v[0] = silu_s(v[0]); v[1] = silu_s(v[1]); v[2] = silu_s(v[2]); v[3] = silu_s(v[3]);
      }
      *reinterpret_cast<f32x4*>(sx + pix * CP + c4 * 4) = v;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const float* xp = sx + ((py + t / 3) * TI + px + t % 3) * CP;
      const float* wt = w + (size_t)__builtin_amdgcn_readfirstlane((t * Cin + c0) * Z2);
#pragma unroll
      for (int k4 = 0; k4 < CK / 4; ++k4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xp + k4 * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int j = 0; j < Z2; ++j) acc[j] = fmaf(v[e], wt[(k4 * 4 + e) * Z2 + j], acc[j]);
      }
    }
  }
  const int oy = ty * T + py, ox = tx * T + px;
  if (oy >= H || ox >= W) return;
#pragma unroll
  for (int j = 0; j < Z2; ++j) acc[j] += bias[j];
  const int E = E2 / 2;
#pragma unroll
  for (int e = 0; e < 4; ++e) {   // emb_channels <= 4
    if (e >= E) break;
    float mu = qb[e], lv = qb[E + e];
#pragma unroll
    for (int j = 0; j < Z2; ++j) { mu = fmaf(qw[e * Z2 + j], acc[j], mu); lv = fmaf(qw[(E + e) * Z2 + j], acc[j], lv); }
    lv = fminf(fmaxf(lv, -30.0f), 20.0f);
    const size_t i = (((size_t)b * E + e) * H + oy) * W + ox;
    if (mean) mean[i] = mu;
    if (log_var) log_var[i] = lv;
    if (z) z[i] = gaussian_sample1(mu, lv, noise_at(noise, i, seed, sid, off), scale);
  }
}

int launch_ae_tail(const float* x, const float* sc, const float* sh, const float* w, const float* bias, const float* qw, const float* qb, int z2,
                   int e2, const float* noise, uint64_t seed, uint64_t sid, uint64_t off, float scale, float* z, float* mean, float* log_var,
                   int batch, int cin, int h, int w_, hipStream_t stream) {
  PF_REQUIRE(z2 >= 2 && z2 <= 8 && z2 % 2 == 0 && e2 >= 2 && e2 <= 8 && e2 % 2 == 0 && cin % 16 == 0, "ae_tail: unsupported channel counts %d->%d->%d", cin, z2, e2);
  PF_REQUIRE(x && sc && sh && w && bias && qw && qb && (z || mean || log_var), "ae_tail: null argument");
  const int grid = batch * cdiv(h, 16) * cdiv(w_, 16);
#define PF_AE_TAIL(Z2) hipLaunchKernelGGL(ae_tail_kernel<Z2>, dim3(grid), dim3(256), 0, stream, x, sc, sh, w, bias, qw, qb, e2, noise, seed, sid, off, \
                                          scale, z, mean, log_var, batch, cin, h, w_)
  switch (z2) {
    case 2: PF_AE_TAIL(2); break;
    case 4: PF_AE_TAIL(4); break;
    case 6: PF_AE_TAIL(6); break;
    default: PF_AE_TAIL(8); break;
  }
#undef PF_AE_TAIL
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}

// Decoder front (latent_diffusion.py:122-129, autoencoder.py:76-79, 281): h = conv_in(post_quant_conv(z / scale)); z NCHW [B][E][H][W], h NHWC
// [B][H][W][C].  thread = (pixel, 4 output channels), as conv_in_kernel; the 1x1 conv (E -> ZC, with its bias) is evaluated for each of the
// pixel's nine taps INSIDE the image only: the reference pads the 1x1's output, so a tap outside contributes zero, not the 1x1's bias.
// conv_in weights [C][ZC][3][3] through LDS, the 1x1's through wave-uniform (scalar) loads.
__global__ __launch_bounds__(256) void ae_front_kernel(const float* __restrict__ z, float scale, const float* __restrict__ pw,
                                                       const float* __restrict__ pb, const float* __restrict__ w, const float* __restrict__ bias,
                                                       float* __restrict__ out, int B, int E, int ZC, int C, int H, int W) {
  extern __shared__ float sw[];  // [C][ZC*9]
  const int K = ZC * 9;
  for (int i = threadIdx.x; i < C * K; i += 256) sw[i] = w[i];
  __syncthreads();
  const int CQ = C / 4;
  const size_t total = (size_t)B * H * W * CQ;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int cq = (int)(idx % CQ);
    const size_t pix = idx / CQ;
    const int xw = (int)(pix % W), yh = (int)((pix / W) % H), b = (int)(pix / ((size_t)W * H));
    float acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = bias[cq * 4 + j];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int iy = yh + r - 1;
      if (iy < 0 || iy >= H) continue;
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const int ix = xw + s - 1;
        if (ix < 0 || ix >= W) continue;
        float zin[4] = {0.f, 0.f, 0.f, 0.f};   // emb_channels <= 4
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e < E) zin[e] = z[(((size_t)b * E + e) * H + iy) * W + ix] / scale;
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {        // z_channels <= 4
          if (ci >= ZC) break;
          float v = pb[ci];
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (e < E) v = fmaf(pw[ci * E + e], zin[e], v);
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j] = fmaf(v, sw[(cq * 4 + j) * K + ci * 9 + r * 3 + s], acc[j]);
        }
      }
    }
    *reinterpret_cast<float4*>(out + pix * C + cq * 4) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  }
}

int launch_ae_front(const float* z, float scale, const float* pw, const float* pb, const float* w, const float* bias, float* out, int batch, int emb,
                    int zc, int cout, int h, int w_, hipStream_t stream) {
  PF_REQUIRE(z && pw && pb && w && bias && out && scale != 0.f, "ae_front: bad arguments");
  PF_REQUIRE(emb >= 1 && emb <= 4 && zc >= 1 && zc <= 4 && cout % 4 == 0 && (size_t)cout * zc * 9 * 4 <= 64 * 1024, "ae_front: unsupported channel counts %d->%d->%d",
             emb, zc, cout);
  const size_t total = (size_t)batch * h * w_ * (cout / 4);
  const int grid = (int)min((size_t)4096, (total + 255) / 256);
  hipLaunchKernelGGL(ae_front_kernel, dim3(grid), dim3(256), (size_t)cout * zc * 9 * sizeof(float), stream, z, scale, pw, pb, w, bias, out, batch, emb, zc,
                     cout, h, w_);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}

// ------------------------------------------------------------------ clock probe
// {shader-clock counter, constant-rate reference counter} per XCD at the moment the probe runs: two probes bracketing a stretch of
// stream work give the AVERAGE shader clock of every XCD over it (the part is power-managed: the same binary clocks differently from
// box to box and under different loads, and the eight XCDs have counters - and clocks - of their own, so a begin / end pair must
// come from the same XCD).  s_memtime counts shader cycles, s_memrealtime the fixed reference clock (100 MHz on gfx950; bench.py
// calibrates it against the host clock instead of assuming it).  64 single-wave workgroups are dealt round-robin over the XCDs;
// each writes row XCC_ID of out[8][2] (several per XCD: the last writer wins, they differ by nanoseconds).
__global__ void clock_probe_kernel(unsigned long long* out) {
  if (threadIdx.x != 0) return;
  const unsigned xcc = __builtin_amdgcn_s_getreg((20 /* HW_REG_XCC_ID */) | (0 << 6) | ((4 - 1) << 11)) & 7u;   // bits 3:0 = XCC id
  out[2 * xcc + 0] = __builtin_amdgcn_s_memtime();
  out[2 * xcc + 1] = __builtin_amdgcn_s_memrealtime();
}
int launch_clock_probe(unsigned long long* out2, hipStream_t s) {
  PF_REQUIRE(out2, "clock_probe: null output");
  hipLaunchKernelGGL(clock_probe_kernel, dim3(64), dim3(64), 0, s, out2);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}

// ------------------------------------------------------------------ matrix-pipe probe
// What the bf16 matrix pipe SUSTAINS on this box, as a reference for roofline fractions: one 8-wave workgroup per CU (two waves per SIMD),
// every wave a dependency-free stream of v_mfma_f32_32x32x16_bf16 over four accumulators - 100 % pipe duty - on operands with random signs
// and mantissas.  The part is power-managed: with such operands a full pipe clocks ~1.6 GHz (all-ones operands: ~2.3 GHz), so the
// sustained rate sits well below the nominal 2.5 PFLOP/s (tools/micro/tap_pingpong.hip, profiles/r04_ab_pingpong.md).
// bench.py times a few launches with events; flops per launch = grid x 8 waves x 24 x 32768 x iters.
__global__ __launch_bounds__(512) void mfma_probe_kernel(float* sink, int iters) {
  typedef float f32x16_t __attribute__((ext_vector_type(16)));
  typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
  typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
  f32x16_t acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  unsigned h = (threadIdx.x + 1) * 2654435761u + blockIdx.x * 40503u;
  auto nx = [&]() { h ^= h << 13; h ^= h >> 17; h ^= h << 5; return (h & 0x807f807fu) | 0x3f003f00u; };   // bf16 pairs in +-[0.5, 1)
  bf16x8_t a[4], b[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const u32x4_t ua = {nx(), nx(), nx(), nx()}, ub = {nx(), nx(), nx(), nx()};
    a[i] = __builtin_bit_cast(bf16x8_t, ua); b[i] = __builtin_bit_cast(bf16x8_t, ub);
  }
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < 24; ++i) acc[i & 3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[(i >> 2) & 3], b[(i + (i >> 3)) & 3], acc[i & 3], 0, 0, 0);
  }
  float r = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) r += acc[i][0] + acc[i][7];
  if (r == 12345.678f) sink[0] = r;   // keeps the stream alive; never true in practice
}
int launch_mfma_probe(float* sink, int iters, double* flops, hipStream_t s) {
  PF_REQUIRE(sink && iters > 0 && iters <= (1 << 20), "mfma_probe: bad arguments");
  const int grid = num_cus();
  hipLaunchKernelGGL(mfma_probe_kernel, dim3(grid), dim3(512), 0, s, sink, iters);
  PF_CHECK_HIP(hipGetLastError());
  if (flops) *flops = (double)grid * 8.0 * 24.0 * 32768.0 * iters;
  return PF_OK;
}

// ------------------------------------------------------------------ GRU cell update (torch gate order r, z, n)
// gi = W_ih x_t + b_ih  [B][3H] (row stride ld_gi), gh = W_hh h + b_hh [B][3H]
__global__ void gru_gates_kernel(const float* __restrict__ gi, int ld_gi, const float* __restrict__ gh, float* __restrict__ h,
                                 int ld_h, int B, int H) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * H) return;
  const int b = i / H, j = i % H;
  const float* a = gi + (size_t)b * ld_gi;
  const float* c = gh + (size_t)b * 3 * H;
  const float r = 1.0f / (1.0f + expf(-(a[j] + c[j])));
  const float z = 1.0f / (1.0f + expf(-(a[H + j] + c[H + j])));
  const float nn = tanhf(a[2 * H + j] + r * c[2 * H + j]);
  float* hp = h + (size_t)b * ld_h + j;
  *hp = (1.0f - z) * nn + z * *hp;
}
int launch_gru_gates(const float* gi, int ld_gi, const float* gh, float* h, int ld_h, int batch, int hidden, hipStream_t s) {
  hipLaunchKernelGGL(gru_gates_kernel, dim3(cdiv(batch * hidden, 256)), dim3(256), 0, s, gi, ld_gi, gh, h, ld_h, batch, hidden);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}

// ------------------------------------------------------------------ PianoTree encoder pieces (dl_modules/pianotree_enc.py)
// grid row = (pitch index, 5 duration digits) as floats; its multi-hot form (one-hot pitch over P classes - the pad index P has no
// column - followed by the five digits, :78-95) times note_embedding (:43): out[row][j] = b[j] + W[j][pitch] + sum_k d_k W[j][P+k]
__global__ void pnotree_embed_kernel(const float* __restrict__ grid, const float* __restrict__ w, const float* __restrict__ bias,
                                     float* __restrict__ out, int rows, int E, int P) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * E) return;
  const int row = i / E, j = i % E;
  const float* g = grid + (size_t)row * 6;
  const float* wj = w + (size_t)j * (P + 5);
  const int pitch = (int)g[0];
  float acc = bias[j];
  if (pitch >= 0 && pitch < P) acc += wj[pitch];
  for (int k = 0; k < 5; ++k) acc = fmaf(g[1 + k], wj[P + k], acc);
  out[i] = acc;
}
// notes sounding at a time step = S minus the pad entries (get_len_index_tensor :69-76)
__global__ void pnotree_lengths_kernel(const float* __restrict__ grid, int* __restrict__ lens, int nseq, int S, int pad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nseq) return;
  int n = S;
  for (int k = 0; k < S; ++k) n -= ((int)grid[((size_t)i * S + k) * 6] == pad);
  lens[i] = n;
}
// GRU cell update over packed variable-length sequences (pack_padded_sequence, :104-107): sequence b takes part in `step` only while
// step < lens[b]; its input is element `step` (forward) or lens[b]-1-step (reverse) of gi [N][S][3H]
__global__ void gru_gates_masked_kernel(const float* __restrict__ gi, const float* __restrict__ gh, float* __restrict__ h, int ld_h,
                                        int N, int H, int S, const int* __restrict__ lens, int step, int reverse) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * H) return;
  const int b = i / H, j = i % H;
  const int len = lens[b];
  if (step >= len) return;
  const int t = reverse ? len - 1 - step : step;
  const float* a = gi + ((size_t)b * S + t) * 3 * H;
  const float* c = gh + (size_t)b * 3 * H;
  const float r = 1.0f / (1.0f + expf(-(a[j] + c[j])));
  const float z = 1.0f / (1.0f + expf(-(a[H + j] + c[H + j])));
  const float nn = tanhf(a[2 * H + j] + r * c[2 * H + j]);
  float* hp = h + (size_t)b * ld_h + j;
  *hp = (1.0f - z) * nn + z * *hp;
}
int launch_pnotree_embed(const float* grid, const float* w, const float* bias, float* out, int rows, int emb, int pitch_range, hipStream_t s) {
  hipLaunchKernelGGL(pnotree_embed_kernel, dim3(cdiv(rows * emb, 256)), dim3(256), 0, s, grid, w, bias, out, rows, emb, pitch_range);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}
int launch_pnotree_lengths(const float* grid, int* lens, int nseq, int max_simu_note, int pad, hipStream_t s) {
  hipLaunchKernelGGL(pnotree_lengths_kernel, dim3(cdiv(nseq, 256)), dim3(256), 0, s, grid, lens, nseq, max_simu_note, pad);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}
int launch_gru_gates_masked(const float* gi, const float* gh, float* h, int ld_h, int nseq, int hidden, int seq_len, const int* lens,
                            int step, int reverse, hipStream_t s) {
  hipLaunchKernelGGL(gru_gates_masked_kernel, dim3(cdiv(nseq * hidden, 256)), dim3(256), 0, s, gi, gh, h, ld_h, nseq, hidden, seq_len, lens, step,
                     reverse);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}

// ------------------------------------------------------------------ texture encoder front end
// pr [B,32,128] -> conv(1->C,(4,12),stride(4,1)) -> ReLU -> maxpool(1,4) -> [B,C,8,29] (contiguous; the
// reference then reinterprets this buffer as [B,8,C*29] without a permute - txt_enc.py:27).
__global__ void txt_frontend_kernel(const float* __restrict__ pr, const float* __restrict__ w, const float* __restrict__ bias,
                                    float* __restrict__ out, int B, int C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int total = B * C * 8 * 29;
  if (i >= total) return;
  const int pw = i % 29, row = (i / 29) % 8, ch = (i / (29 * 8)) % C, b = i / (29 * 8 * C);
  const float* src = pr + (size_t)b * 32 * 128 + (size_t)row * 4 * 128;
  const float* wk = w + (size_t)ch * 48;
  float best = 0.f;  // ReLU floor
  for (int q = 0; q < 4; ++q) {
    const int col = pw * 4 + q;
    float acc = bias[ch];
    for (int r = 0; r < 4; ++r)
      for (int s = 0; s < 12; ++s) acc = fmaf(src[r * 128 + col + s], wk[r * 12 + s], acc);
    best = fmaxf(best, acc);
  }
  out[i] = best;
}
int launch_txt_frontend(const float* pr, const float* w, const float* bias, float* out, int batch, int num_channel, hipStream_t s) {
  hipLaunchKernelGGL(txt_frontend_kernel, dim3(cdiv(batch * num_channel * 8 * 29, 256)), dim3(256), 0, s, pr, w, bias, out, batch,
                     num_channel);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}

}  // namespace pf
