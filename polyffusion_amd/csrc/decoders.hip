// decoders.hip - the frozen decoders of Polyffusion_SDF in inference mode (greedy, arg-max fed back), plain fp32.
//   pnotree: PianoTreeDecoder.decoder(z, inference=True, ...)            (dl_modules/pianotree_dec.py:155-332)
//   chord:   ChordDecoder.forward(z_chd, inference=True, tfr=0)          (dl_modules/chord_dec.py:27-70)
//            and the same walk with teacher forcing (inference=False): pf_decoder_forward_forced
// A PianoTree decode is 32 time steps x (max_simu_note - 1) note slots, every slot depending on the arg-max of the one before it.
// Per note slot there are two launches: one fused GRU step (W_hh.h mat-vec with the gate update in its epilogue; a workgroup owns four
// hidden units and eight rows of the batch, so W_hh is read once per slot per 8-row tile) and one "heads" launch (a workgroup per row:
// pitch logits, arg-max, end-token bookkeeping, the 5-step duration GRU, and the next token's contribution to the GRU input, which is
// a gather of at most seven rows of a table formed at bind time: W_ih[:, token part] . note_embedding).  Per time step: the time-GRU
// step, two linear layers and one launch of the bidirectional embedding GRU over each row's own predicted length.  Stream order is the
// only dependency between workgroups.  Every reduction runs over k in an order that depends on neither the row's position in the batch
// nor the batch size.
#include <memory>
#include "plan.h"

using namespace pf;

namespace {

constexpr int RT = 8;          // rows of the batch a workgroup of the mat-vec kernels holds in LDS
constexpr int PN_P = 130;      // pitch classes (128 pitches, sos, eos)
constexpr int PN_DW = 5;       // duration digits
constexpr int PN_TOK = PN_P + PN_DW;   // note token width (135)
constexpr int PN_E = 128;      // note embedding
constexpr int PN_Z = 512, PN_ZIN = 256, PN_HT = 1024, PN_HN = 512, PN_HE = 128;
// (the duration GRU's width, dec_dur_hid_size, is the template parameter HD of the heads kernel: 16 or 64)
constexpr int PN_TROWS = PN_TOK + 1;   // table rows: 135 token columns + the embedding-bias row

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float sigmoid_f(float v) { return 1.0f / (1.0f + expf(-v)); }

// acc[i][r] += sum_k w[i][k] * xs[r][k]: a wave strides k (lane = k / 4 for the vector form), rows of x in LDS
template <int NW, bool VEC>
__device__ __forceinline__ void wave_dot(const float* const (&w)[NW], int K, const float* xs, int ldxs, int lane, float (&acc)[NW][RT]) {
  if (VEC) {
    for (int k = lane * 4; k < K; k += 256) {
      float4 wv[NW];
#pragma unroll
      for (int i = 0; i < NW; ++i) wv[i] = *reinterpret_cast<const float4*>(w[i] + k);
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        const float4 xv = *reinterpret_cast<const float4*>(xs + r * ldxs + k);
#pragma unroll
        for (int i = 0; i < NW; ++i)
          acc[i][r] = fmaf(wv[i].w, xv.w, fmaf(wv[i].z, xv.z, fmaf(wv[i].y, xv.y, fmaf(wv[i].x, xv.x, acc[i][r]))));
      }
    }
  } else {
    for (int k = lane; k < K; k += 64) {
      float wv[NW];
#pragma unroll
      for (int i = 0; i < NW; ++i) wv[i] = w[i][k];
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        const float xv = xs[r * ldxs + k];
#pragma unroll
        for (int i = 0; i < NW; ++i) acc[i][r] = fmaf(wv[i], xv, acc[i][r]);
      }
    }
  }
}

// rows r0 .. r0+RT-1 of x [R][ldx] -> LDS [RT][K] (rows past R are zero)
__device__ __forceinline__ void stage_rows(const float* x, int ldx, int K, int r0, int R, float* xs) {
  for (int i = threadIdx.x; i < RT * K; i += blockDim.x) {
    const int r = i / K, k = i - r * K;
    xs[i] = (r0 + r < R) ? x[(size_t)(r0 + r) * ldx + k] : 0.f;
  }
}

// y[r][n] = sum_k W[n][k] x[r][k] + bias[n]; W rows ldw apart (a column slice of a wider matrix is allowed).  A wave per output.
__global__ __launch_bounds__(256) void dec_linear_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w, int ldw,
                                                         const float* __restrict__ bias, float* __restrict__ y, int ldy, int R, int N,
                                                         int K, int vec) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = blockIdx.y * RT;
  stage_rows(x, ldx, K, r0, R, lds);
  __syncthreads();
  const int n = blockIdx.x * 4 + wave;
  if (n >= N) return;
  float acc[1][RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) acc[0][r] = 0.f;
  const float* const wr[1] = {w + (size_t)n * ldw};
  if (vec) wave_dot<1, true>(wr, K, lds, K, lane, acc);
  else wave_dot<1, false>(wr, K, lds, K, lane, acc);
  const float b = bias ? bias[n] : 0.f;
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    const float v = wave_sum(acc[0][r]);
    if (lane == r && r0 + r < R) y[(size_t)(r0 + r) * ldy + n] = v + b;
  }
}

// One GRU step for every row of the batch (torch.nn.GRU cell, gates r | z | n):
//   gi = Wx . x + add1 + add2      (x: the part of the input that changes per step; add1 / add2: hoisted parts, bias_ih included)
//   gh = Wh . h_in + b_hh
//   h_out = (1 - z) * tanh(gi_n + r * gh_n) + z * h_in
// A wave owns hidden unit j (its three gate rows), a workgroup four units and RT rows of the batch.  h_in and h_out are two buffers:
// other workgroups still read h_in while this one writes.
struct GruStepArgs {
  const float* x; int ldx, Kx; const float* wx; int ldwx;
  const float* h_in; const float* wh; const float* b_hh;
  const float* add1; int ld1; const float* add2; int ld2;
  float* h_out; int R, H;
};
__global__ __launch_bounds__(256) void gru_step_kernel(GruStepArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* hs = lds;                     // [RT][H]
  float* xs = lds + RT * a.H;          // [RT][Kx]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = blockIdx.y * RT, H = a.H;
  stage_rows(a.h_in, H, H, r0, a.R, hs);
  if (a.Kx > 0) stage_rows(a.x, a.ldx, a.Kx, r0, a.R, xs);
  __syncthreads();
  const int j = blockIdx.x * 4 + wave;
  if (j >= H) return;
  float gh[3][RT], gi[3][RT];
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int r = 0; r < RT; ++r) { gh[g][r] = 0.f; gi[g][r] = 0.f; }
  const float* const whr[3] = {a.wh + (size_t)j * H, a.wh + (size_t)(H + j) * H, a.wh + (size_t)(2 * H + j) * H};
  wave_dot<3, true>(whr, H, hs, H, lane, gh);          // H % 4 == 0 and the blob is 256-byte aligned: checked at create / bind
  if (a.Kx > 0) {
    const float* const wxr[3] = {a.wx + (size_t)j * a.ldwx, a.wx + (size_t)(H + j) * a.ldwx, a.wx + (size_t)(2 * H + j) * a.ldwx};
    wave_dot<3, false>(wxr, a.Kx, xs, a.Kx, lane, gi);
  }
  const float bhr = a.b_hh[j], bhz = a.b_hh[H + j], bhn = a.b_hh[2 * H + j];
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    const float hr = wave_sum(gh[0][r]), hz = wave_sum(gh[1][r]), hn = wave_sum(gh[2][r]);
    const float ir = wave_sum(gi[0][r]), iz = wave_sum(gi[1][r]), in = wave_sum(gi[2][r]);
    if (lane == r && r0 + r < a.R) {
      const int row = r0 + r;
      float cr = ir, cz = iz, cn = in;
      if (a.add1) { const float* p = a.add1 + (size_t)row * a.ld1; cr += p[j]; cz += p[H + j]; cn += p[2 * H + j]; }
      if (a.add2) { const float* p = a.add2 + (size_t)row * a.ld2; cr += p[j]; cz += p[H + j]; cn += p[2 * H + j]; }
      const float rg = sigmoid_f(cr + (hr + bhr));
      const float zg = sigmoid_f(cz + (hz + bhz));
      const float ng = tanhf(cn + rg * (hn + bhn));
      a.h_out[(size_t)row * H + j] = (1.0f - zg) * ng + zg * hs[r * H + j];
    }
  }
}

// ---- PianoTree heads: one workgroup per row, one note slot (decode_note + the bookkeeping of decode_notes, pianotree_dec.py:155-244)
// HD = dec_dur_hid_size.  At 16 a thread per hidden unit walks its three rows of the duration GRU's W_hh (48 x 16 floats, in cache).  At 64
// that walk would be 64 threads striding 64 floats apart, five times per slot, so the 192 gate rows get a thread each instead: W_hh is
// read in a transposed copy made at bind time (consecutive threads, consecutive addresses: the form of pnotree_emb_gru_kernel), a
// thread keeps its column in registers over the five digits, and the two output logits are one wave-wide product each.  k runs 0..63 in
// a thread (gates) or over the fixed butterfly of wave_sum (logits): the same order for every row of every batch.
struct PnHeadsArgs {
  const float* h;                                    // [R][512] the notes-GRU output of this slot
  const float *wp, *bp;                              // pitch_out_linear [130][512]
  const float *wdh, *bdh;                            // dur_hid_linear [HD][512 + 130]
  const float *wdi, *wdhh, *bdi, *bdhh;              // dec_dur_gru [3 HD][5] [3 HD][HD] [3 HD] [3 HD]
  const float *wdo, *bdo;                            // dur_out_linear [2][HD]
  const float* dur_sos;                              // [5]
  const float *tn, *te;                              // token tables [136][1536] (notes GRU) and [136][768] (embedding GRU, both directions)
  float *recon_pitch, *recon_dur; int32_t* est;      // [R][32][S-1][130], [R][32][S-1][5][2], [R][32][S-1][6]
  float *gi_tok, *gie; int* lens;                    // [R][1536], [R][S][768], [R]
  int t, s, S;
  const float* wdhh_t;                               // HD = 64: dec_dur_gru.weight_hh_l0 transposed, [64][192]
};
template <int HD>
__global__ __launch_bounds__(256) void pnotree_heads_kernel(PnHeadsArgs a) {
  static_assert(HD == 16 || HD == 64, "the duration GRU is 16 or 64 wide");
  constexpr int PN_HD = HD;
  __shared__ __attribute__((aligned(16))) float hs[PN_HN + PN_P];   // [note_summary | est_pitch]: the input of dur_hid_linear
  __shared__ float dh[PN_HD], dl[2];
  __shared__ float gs[HD == 64 ? 3 * HD : 1], is[HD == 64 ? 3 * HD : 1];   // HD = 64: the gate rows' hidden / input parts
  __shared__ int pidx;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = blockIdx.x;
  const size_t slot = ((size_t)row * 32 + a.t) * (a.S - 1) + (a.s - 1);
  for (int k = tid; k < PN_HN; k += 256) hs[k] = a.h[(size_t)row * PN_HN + k];
  __syncthreads();
  for (int o = wave; o < PN_P; o += 4) {
    const float* wr = a.wp + (size_t)o * PN_HN;
    float acc = 0.f;
#pragma unroll
    for (int k = lane * 4; k < PN_HN; k += 256) {
      const float4 wv = *reinterpret_cast<const float4*>(wr + k);
      const float4 xv = *reinterpret_cast<const float4*>(hs + k);
      acc = fmaf(wv.w, xv.w, fmaf(wv.z, xv.z, fmaf(wv.y, xv.y, fmaf(wv.x, xv.x, acc))));
    }
    acc = wave_sum(acc) + a.bp[o];
    if (lane == 0) { hs[PN_HN + o] = acc; a.recon_pitch[slot * PN_P + o] = acc; }
  }
  __syncthreads();
  if (wave == 0) {   // arg-max of 130, ties to the lowest index
    float bv = hs[PN_HN + lane];
    int bi = lane;
    for (int o = lane + 64; o < PN_P; o += 64) {
      const float v = hs[PN_HN + o];
      if (v > bv) { bv = v; bi = o; }
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
      const float ov = __shfl_xor(bv, off);
      const int oi = __shfl_xor(bi, off);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) pidx = bi;
  }
  for (int o = wave; o < PN_HD; o += 4) {   // dur_hid_linear
    const float* wr = a.wdh + (size_t)o * (PN_HN + PN_P);
    float acc = 0.f;
    for (int k = lane; k < PN_HN + PN_P; k += 64) acc = fmaf(wr[k], hs[k], acc);
    acc = wave_sum(acc) + a.bdh[o];
    if (lane == 0) dh[o] = acc;
  }
  __syncthreads();
  const int pitch = pidx;
  int digit[PN_DW];
  int prev = 0;
  if constexpr (HD == 64) {
    float wcol[HD];                    // this gate row of W_hh, kept over the five digits
    float bh = 0.f, bi = 0.f;
    if (tid < 3 * HD) {
#pragma unroll
      for (int k = 0; k < HD; ++k) wcol[k] = a.wdhh_t[k * (3 * HD) + tid];
      bh = a.bdhh[tid];
      bi = a.bdi[tid];
    }
#pragma unroll
    for (int d = 0; d < PN_DW; ++d) {
      if (tid < 3 * HD) {
        float g = bh;
#pragma unroll
        for (int k = 0; k < HD; ++k) g = fmaf(wcol[k], dh[k], g);
        float i = bi;
        if (d == 0) {
          for (int k = 0; k < PN_DW; ++k) i = fmaf(a.wdi[tid * PN_DW + k], a.dur_sos[k], i);
        } else {
          i += a.wdi[tid * PN_DW + prev];
        }
        gs[tid] = g;
        is[tid] = i;
      }
      __syncthreads();
      if (tid < HD) {
        const float rg = sigmoid_f(is[tid] + gs[tid]), zg = sigmoid_f(is[HD + tid] + gs[HD + tid]);
        const float ng = tanhf(is[2 * HD + tid] + rg * gs[2 * HD + tid]);
        dh[tid] = (1.0f - zg) * ng + zg * dh[tid];
      }
      __syncthreads();
      if (wave < 2) {                  // HD == 64 == a wave: one product per lane
        const float l = wave_sum(a.wdo[wave * HD + lane] * dh[lane]) + a.bdo[wave];
        if (lane == 0) {
          dl[wave] = l;
          a.recon_dur[(slot * PN_DW + d) * 2 + wave] = l;
        }
      }
      __syncthreads();
      prev = dl[1] > dl[0] ? 1 : 0;
      digit[d] = prev;
    }
  } else {
#pragma unroll
  for (int d = 0; d < PN_DW; ++d) {   // dec_dur_gru + dur_out_linear, the arg-max fed back as a one-hot of width 5
    float hn = 0.f;
    if (tid < PN_HD) {
      float gr = a.bdhh[tid], gz = a.bdhh[PN_HD + tid], gn = a.bdhh[2 * PN_HD + tid];
      for (int k = 0; k < PN_HD; ++k) {
        const float hk = dh[k];
        gr = fmaf(a.wdhh[tid * PN_HD + k], hk, gr);
        gz = fmaf(a.wdhh[(PN_HD + tid) * PN_HD + k], hk, gz);
        gn = fmaf(a.wdhh[(2 * PN_HD + tid) * PN_HD + k], hk, gn);
      }
      float ir = a.bdi[tid], iz = a.bdi[PN_HD + tid], in = a.bdi[2 * PN_HD + tid];
      if (d == 0) {
        for (int k = 0; k < PN_DW; ++k) {
          const float tk = a.dur_sos[k];
          ir = fmaf(a.wdi[tid * PN_DW + k], tk, ir);
          iz = fmaf(a.wdi[(PN_HD + tid) * PN_DW + k], tk, iz);
          in = fmaf(a.wdi[(2 * PN_HD + tid) * PN_DW + k], tk, in);
        }
      } else {
        ir += a.wdi[tid * PN_DW + prev];
        iz += a.wdi[(PN_HD + tid) * PN_DW + prev];
        in += a.wdi[(2 * PN_HD + tid) * PN_DW + prev];
      }
      const float rg = sigmoid_f(ir + gr), zg = sigmoid_f(iz + gz);
      const float ng = tanhf(in + rg * gn);
      hn = (1.0f - zg) * ng + zg * dh[tid];
    }
    __syncthreads();
    if (tid < PN_HD) dh[tid] = hn;
    __syncthreads();
    if (tid < 2) {
      float l = a.bdo[tid];
      for (int k = 0; k < PN_HD; ++k) l = fmaf(a.wdo[tid * PN_HD + k], dh[k], l);
      dl[tid] = l;
      a.recon_dur[(slot * PN_DW + d) * 2 + tid] = l;
    }
    __syncthreads();
    prev = dl[1] > dl[0] ? 1 : 0;
    digit[d] = prev;
  }
  }
  if (tid == 0) {
    int32_t* e = a.est + slot * 6;
    e[0] = pitch;
#pragma unroll
    for (int d = 0; d < PN_DW; ++d) e[1 + d] = digit[d];
    // lengths[eos & lengths == 0] = s; lengths[lengths == 0] = S - 1 after the last slot (pianotree_dec.py:234-244)
    int len = a.s == 1 ? 0 : a.lens[row];
    if (pitch == PN_P - 1 && len == 0) len = a.s;
    if (a.s == a.S - 1 && len == 0) len = a.S - 1;
    a.lens[row] = len;
  }
  // the predicted token (one-hot pitch | duration digits) through note_embedding and the input weights: a gather of table rows
  if (a.s < a.S - 1) {
    for (int j = tid; j < 3 * PN_HN; j += 256) {
      float v = a.tn[(size_t)pitch * (3 * PN_HN) + j];
#pragma unroll
      for (int d = 0; d < PN_DW; ++d)
        if (digit[d]) v += a.tn[(size_t)(PN_P + d) * (3 * PN_HN) + j];
      a.gi_tok[(size_t)row * (3 * PN_HN) + j] = v + a.tn[(size_t)PN_TOK * (3 * PN_HN) + j];
    }
  }
  for (int j = tid; j < 6 * PN_HE; j += 256) {
    float v = a.te[(size_t)pitch * (6 * PN_HE) + j];
#pragma unroll
    for (int d = 0; d < PN_DW; ++d)
      if (digit[d]) v += a.te[(size_t)(PN_P + d) * (6 * PN_HE) + j];
    a.gie[((size_t)row * a.S + a.s) * (6 * PN_HE) + j] = v + a.te[(size_t)PN_TOK * (6 * PN_HE) + j];
  }
}

// dec_notes_emb_gru over [sos, predicted notes ...] of each row, up to the row's own predicted length (pack_padded_sequence: the final
// hidden state of each direction at that length).  A workgroup per (row, direction), 384 threads = the gate rows; W_hh is read in its
// transposed copy so that the threads of a wave read consecutive addresses.  out[row] = [h_forward | h_backward].
__global__ __launch_bounds__(3 * PN_HE) void pnotree_emb_gru_kernel(const float* __restrict__ gie, const float* __restrict__ gie_sos,
                                                                    const float* __restrict__ whh_t, const float* __restrict__ bhh_f,
                                                                    const float* __restrict__ bhh_b, const int* __restrict__ lens,
                                                                    float* __restrict__ out, int S) {
  __shared__ float hs[PN_HE], gs[3 * PN_HE], is[3 * PN_HE];
  const int tid = threadIdx.x, row = blockIdx.x, dir = blockIdx.y;
  const int L = min(max(lens[row], 0), S - 1);
  const float* wt = whh_t + (size_t)dir * PN_HE * 3 * PN_HE;
  const float bh = (dir ? bhh_b : bhh_f)[tid];
  if (tid < PN_HE) hs[tid] = 0.f;
  __syncthreads();
  for (int i = 0; i < L; ++i) {
    const int idx = dir ? L - 1 - i : i;
    const float* gi = idx == 0 ? gie_sos : gie + ((size_t)row * S + idx) * (6 * PN_HE);
    float acc = 0.f;
#pragma unroll 8
    for (int k = 0; k < PN_HE; ++k) acc = fmaf(wt[k * (3 * PN_HE) + tid], hs[k], acc);
    gs[tid] = acc + bh;
    is[tid] = gi[dir * 3 * PN_HE + tid];
    __syncthreads();
    if (tid < PN_HE) {
      const float rg = sigmoid_f(is[tid] + gs[tid]);
      const float zg = sigmoid_f(is[PN_HE + tid] + gs[PN_HE + tid]);
      const float ng = tanhf(is[2 * PN_HE + tid] + rg * gs[2 * PN_HE + tid]);
      hs[tid] = (1.0f - zg) * ng + zg * hs[tid];
    }
    __syncthreads();
  }
  if (tid < PN_HE) out[(size_t)row * 2 * PN_HE + dir * PN_HE + tid] = hs[tid];
}

// ---- chord heads: root 12 | chroma 12x2 | bass 12 logits of one step, and the next token one-hot root | chroma bits | one-hot bass
// (chord_dec.py:39-64).  One workgroup per row.  forced (teacher forcing, chord_dec.py:56-57): the row's ground-truth token of this step,
// rows ld_forced apart, written as the next token instead of the arg-max one; null on the greedy path.
__global__ __launch_bounds__(256) void chord_heads_kernel(const float* __restrict__ h, int H, const float* __restrict__ w_root,
                                                          const float* __restrict__ b_root, const float* __restrict__ w_chroma,
                                                          const float* __restrict__ b_chroma, const float* __restrict__ w_bass,
                                                          const float* __restrict__ b_bass, float* __restrict__ root,
                                                          float* __restrict__ chroma, float* __restrict__ bass, float* __restrict__ token,
                                                          int t, int n_step, const float* __restrict__ forced, int ld_forced) {
  __shared__ float hs[1024], lg[48];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = blockIdx.x;
  for (int k = tid; k < H; k += 256) hs[k] = h[(size_t)row * H + k];
  __syncthreads();
  const size_t step = (size_t)row * n_step + t;
  for (int o = wave; o < 48; o += 4) {
    const float* wr = o < 12 ? w_root + (size_t)o * H : (o < 36 ? w_chroma + (size_t)(o - 12) * H : w_bass + (size_t)(o - 36) * H);
    float acc = 0.f;
    for (int k = lane; k < H; k += 64) acc = fmaf(wr[k], hs[k], acc);
    acc = wave_sum(acc) + (o < 12 ? b_root[o] : (o < 36 ? b_chroma[o - 12] : b_bass[o - 36]));
    if (lane == 0) {
      lg[o] = acc;
      if (o < 12) root[step * 12 + o] = acc;
      else if (o < 36) chroma[step * 24 + (o - 12)] = acc;
      else bass[step * 12 + (o - 36)] = acc;
    }
  }
  __syncthreads();
  if (tid < 36) {
    float v;
    if (tid >= 12 && tid < 24) {
      v = lg[12 + 2 * (tid - 12) + 1] > lg[12 + 2 * (tid - 12)] ? 1.f : 0.f;
    } else {
      const float* p = tid < 12 ? lg : lg + 36;
      int bi = 0;
      for (int o = 1; o < 12; ++o)
        if (p[o] > p[bi]) bi = o;
      v = (tid < 12 ? tid : tid - 24) == bi ? 1.f : 0.f;
    }
    token[(size_t)row * 36 + tid] = forced ? forced[(size_t)row * ld_forced + tid] : v;
  }
}

// The reference's fed-back token at batch > 1 (chord_dec.py:59-63): t_root[arange(bs), 0, idx] with idx of shape (bs, 1) sets, in EVERY
// row, the root (and bass) columns of ALL rows' arg-maxes.  Token entries are 0 / 1, so that union is a maximum over the call's rows;
// the chroma bits stay the row's own.  One wave per root / bass column: its lanes stride the rows, combine by a butterfly (a maximum of
// 0 / 1 values: no order to keep) and write the column back.  No workgroup touches another's column.
__global__ __launch_bounds__(64) void chord_union_kernel(float* __restrict__ token, int R) {
  const int col = blockIdx.x < 12 ? blockIdx.x : blockIdx.x + 12, lane = threadIdx.x;
  float m = 0.f;
  for (int r = lane; r < R; r += 64) m = fmaxf(m, token[(size_t)r * 36 + col]);
#pragma unroll
  for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  for (int r = lane; r < R; r += 64) token[(size_t)r * 36 + col] = m;
}

// ---- bind-time tables
// out[c][off + j] = sum_e W[j][col + e] * emb_w[e][c]  (c < 135);   out[135][off + j] = sum_e W[j][col + e] * emb_b[e] + bias[j]
__global__ void token_table_kernel(const float* __restrict__ w, int ldw, int col, int n, const float* __restrict__ emb_w,
                                   const float* __restrict__ emb_b, const float* __restrict__ bias, float* __restrict__ out, int ld_out,
                                   int off) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
  if (j >= n) return;
  const float* wr = w + (size_t)j * ldw + col;
  float acc = 0.f;
  if (c < PN_TOK) {
    for (int e = 0; e < PN_E; ++e) acc = fmaf(wr[e], emb_w[e * PN_TOK + c], acc);
  } else {
    for (int e = 0; e < PN_E; ++e) acc = fmaf(wr[e], emb_b[e], acc);
    if (bias) acc += bias[j];
  }
  out[(size_t)c * ld_out + off + j] = acc;
}
// the start token (get_sos_token: one-hot pitch_sos, duration part 2.0) through a table
__global__ void sos_row_kernel(const float* __restrict__ tab, int n, float* __restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  float v = tab[(size_t)(PN_P - 2) * n + j];
  for (int d = 0; d < PN_DW; ++d) v = fmaf(2.0f, tab[(size_t)(PN_P + d) * n + j], v);
  out[j] = v + tab[(size_t)PN_TOK * n + j];
}
__global__ void transpose_kernel(const float* __restrict__ w, int rows, int cols, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * cols) return;
  const int r = i / cols, c = i - r * cols;
  out[(size_t)c * rows + r] = w[i];
}

int launched() {   // after a hipLaunchKernelGGL
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}
int launch_linear(const float* x, int ldx, const float* w, int ldw, const float* bias, float* y, int ldy, int R, int N, int K,
                  hipStream_t s) {
  PF_REQUIRE(K <= 2048, "decoder linear: K=%d too large", K);
  const int vec = (K % 4 == 0) && (ldw % 4 == 0) && (((uintptr_t)w & 15) == 0);
  hipLaunchKernelGGL(dec_linear_kernel, dim3(cdiv(N, 4), cdiv(R, RT)), dim3(256), (size_t)RT * K * sizeof(float), s, x, ldx, w, ldw, bias,
                     y, ldy, R, N, K, vec);
  return launched();
}
int launch_gru_step(const GruStepArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(gru_step_kernel, dim3(cdiv(a.H, 4), cdiv(a.R, RT)), dim3(256), (size_t)RT * (a.H + a.Kx) * sizeof(float), s, a);
  return launched();
}

}  // namespace

// pf_gru_step: the kernel alone, with everything the decode walk guarantees by construction checked here
int pf::launch_gru_step_flat(const pf_gru_step_args& f, hipStream_t s) {
  PF_REQUIRE(f.h_in && f.wh && f.b_hh && f.h_out && f.R > 0 && f.H > 0 && f.Kx >= 0, "pf_gru_step: bad arguments");
  PF_REQUIRE(f.H % 4 == 0, "pf_gru_step: H=%d must be a multiple of 4", f.H);
  PF_REQUIRE(((uintptr_t)f.wh & 15) == 0 && ((uintptr_t)f.h_in & 15) == 0, "pf_gru_step: wh and h_in must be 16-byte aligned");
  PF_REQUIRE((size_t)RT * ((size_t)f.H + f.Kx) * sizeof(float) <= 64 * 1024, "pf_gru_step: H=%d + Kx=%d rows of 8 do not fit 64 KiB", f.H, f.Kx);
  PF_REQUIRE(f.h_out != f.h_in, "pf_gru_step: h_out must not be h_in (other workgroups still read it)");
  PF_REQUIRE(f.Kx == 0 || (f.x && f.wx && f.ldwx >= f.Kx && (f.ldx == 0 || f.ldx >= f.Kx)), "pf_gru_step: bad x / wx");
  PF_REQUIRE((!f.add1 || f.ld1 == 0 || f.ld1 >= 3 * f.H) && (!f.add2 || f.ld2 == 0 || f.ld2 >= 3 * f.H), "pf_gru_step: bad add1 / add2 stride");
  GruStepArgs a;
  a.x = f.x; a.ldx = f.ldx; a.Kx = f.Kx; a.wx = f.wx; a.ldwx = f.ldwx;
  a.h_in = f.h_in; a.wh = f.wh; a.b_hh = f.b_hh;
  a.add1 = f.add1; a.ld1 = f.ld1; a.add2 = f.add2; a.ld2 = f.ld2;
  a.h_out = f.h_out; a.R = f.R; a.H = f.H;
  return launch_gru_step(a, s);
}

struct pf_decoder {
  int kind = 0;
  int S = 0, HD = 16;                                          // pnotree: max_simu_note, dec_dur_hid_size
  int input_dim = 0, z_input_dim = 0, hidden = 0, z_dim = 0, n_step = 0;   // chord
  WeightTable wt;
  // blob offsets of everything forward and bind read, resolved at create
  size_t init_input = 0;                                       // dec_init_input / init_input
  LinOff z2hid{}, z2in{};                                      // z2dec_hid(_linear), z2dec_in(_linear)
  GruOff gru{};                                                // dec_time_gru / the chord decoder's gru
  LinOff root{}, chroma{}, bass{};                             // chord heads
  size_t dur_sos = 0;                                          // pnotree from here on
  LinOff note_emb{}, t2n{}, pitch{}, dur_hid{}, dur_out{};
  GruOff emb_gru[2] = {}, notes_gru{}, dur_gru{};
  size_t tn = 0, te = 0, tn_sos = 0, te_sos = 0, whh_t = 0;   // bind-time tables
  size_t wdhh_t = 0;                                           // HD = 64: transposed dec_dur_gru.weight_hh_l0
};

namespace {

// teacher forcing of the chord walk: bit t of mask set = the token fed to step t + 1 is gt[:, t] (gt [R][n_step][36]); null = greedy
struct ChordForce { const float* gt; uint64_t mask; int feedback; };

// The decode of either kind, dry or live (c.B = rows).  The two halves of a ping-pong buffer are told apart inside the closures: a
// dry run carries null pointers and does no arithmetic on them.
int dec_run(const pf_decoder* d, PlanCtx& c, const float* z, float* out0, float* out1, float* out2, int32_t* est,
            const ChordForce* force = nullptr) {
  const int R = c.B;
  // one fused GRU step h[cur] -> h[cur ^ 1] of the ping-pong pair h [2][R][H]
  auto gru_step = [&](const GruOff& g, const float* x, int ldx, int Kx, int ldwx, float* h, int cur, int H, const float* add1, const float* add2, int ld2) {
    c.launch(PF_K_SMALL, 0.0, [&] {
      GruStepArgs a;
      a.x = x; a.ldx = ldx; a.Kx = Kx; a.wx = Kx ? c.w(g.w_ih) : nullptr; a.ldwx = ldwx;
      a.h_in = h + (size_t)cur * R * H; a.wh = c.w(g.w_hh); a.b_hh = c.w(g.b_hh);
      a.add1 = add1; a.ld1 = 3 * H; a.add2 = add2; a.ld2 = ld2;
      a.h_out = h + (size_t)(cur ^ 1) * R * H; a.R = R; a.H = H;
      return launch_gru_step(a, c.s);
    });
  };
  auto linear = [&](const float* x, int ldx, size_t w, int ldw, size_t bias, float* y, int N, int K) {
    c.launch(PF_K_SMALL, 0.0, [&] { return launch_linear(x, ldx, c.w(w), ldw, c.w(bias), y, N, R, N, K, c.s); });
  };
  if (d->kind == PF_DEC_CHORD) {
    const int H = d->hidden, ZI = d->z_input_dim, IN = d->input_dim, ldw = IN + ZI;
    float* h = c.palloc((size_t)2 * R * H);
    float* z_in = c.palloc((size_t)R * ZI);
    float* gi_z = c.palloc((size_t)R * 3 * H);
    float* token = c.palloc((size_t)R * 36);
    linear(z, d->z_dim, d->z2hid.w, d->z_dim, d->z2hid.b, h, H, d->z_dim);
    linear(z, d->z_dim, d->z2in.w, d->z_dim, d->z2in.b, z_in, ZI, d->z_dim);
    // the z_in part of the GRU input is the same at every step: applied once (bias_ih included)
    linear(z_in, ZI, d->gru.w_ih + IN, ldw, d->gru.b_ih, gi_z, 3 * H, ZI);
    for (int t = 0; t < d->n_step; ++t) {
      gru_step(d->gru, t == 0 ? c.w(d->init_input) : token, t == 0 ? 0 : 36, IN, ldw, h, t & 1, H, gi_z, nullptr, 0);
      const bool fed = t < d->n_step - 1;   // a token follows this step
      const bool forced = force && fed && ((force->mask >> t) & 1);
      c.launch(PF_K_SMALL, 0.0, [&] {
        const float* gt_t = forced ? force->gt + (size_t)t * 36 : nullptr;
        hipLaunchKernelGGL(chord_heads_kernel, dim3(R), dim3(256), 0, c.s, (const float*)(h + (size_t)((t + 1) & 1) * R * H), H, c.w(d->root.w),
                           c.w(d->root.b), c.w(d->chroma.w), c.w(d->chroma.b), c.w(d->bass.w), c.w(d->bass.b), out0, out1, out2, token, t,
                           d->n_step, gt_t, d->n_step * 36);
        return launched();
      });
      if (force && force->feedback == PF_FEEDBACK_BATCH && fed && !forced)
        c.launch(PF_K_SMALL, 0.0, [&] {
          hipLaunchKernelGGL(chord_union_kernel, dim3(24), dim3(64), 0, c.s, token, R);
          return launched();
        });
    }
    return c.rc;
  }
  const int S = d->S;
  float* ht = c.palloc((size_t)2 * R * PN_HT);
  float* z_in = c.palloc((size_t)R * PN_ZIN);
  float* gi_z = c.palloc((size_t)R * 3 * PN_HT);
  float* tok_t = c.palloc((size_t)R * 2 * PN_HE);
  float* hn = c.palloc((size_t)2 * R * PN_HN);
  float* gi_ns = c.palloc((size_t)R * 3 * PN_HN);
  float* gi_tok = c.palloc((size_t)R * 3 * PN_HN);
  float* gie = c.palloc((size_t)R * S * 6 * PN_HE);
  int* lens = reinterpret_cast<int*>(c.palloc(R));
  const int ldt = PN_ZIN + 2 * PN_HE, ldn = PN_HT + PN_E;
  linear(z, PN_Z, d->z2hid.w, PN_Z, d->z2hid.b, ht, PN_HT, PN_Z);
  linear(z, PN_Z, d->z2in.w, PN_Z, d->z2in.b, z_in, PN_ZIN, PN_Z);
  // dec_time_gru input = [token | z_in] (pianotree_dec.py:286-288): the z_in half is constant over the 32 steps
  linear(z_in, PN_ZIN, d->gru.w_ih + 2 * PN_HE, ldt, d->gru.b_ih, gi_z, 3 * PN_HT, PN_ZIN);
  PnHeadsArgs ha;
  ha.wp = c.w(d->pitch.w); ha.bp = c.w(d->pitch.b);
  ha.wdh = c.w(d->dur_hid.w); ha.bdh = c.w(d->dur_hid.b);
  ha.wdi = c.w(d->dur_gru.w_ih); ha.wdhh = c.w(d->dur_gru.w_hh);
  ha.bdi = c.w(d->dur_gru.b_ih); ha.bdhh = c.w(d->dur_gru.b_hh);
  ha.wdhh_t = d->HD == 64 ? c.w(d->wdhh_t) : nullptr;
  ha.wdo = c.w(d->dur_out.w); ha.bdo = c.w(d->dur_out.b);
  ha.dur_sos = c.w(d->dur_sos);
  ha.tn = c.w(d->tn); ha.te = c.w(d->te);
  ha.recon_pitch = out0; ha.recon_dur = out1; ha.est = est;
  ha.gi_tok = gi_tok; ha.gie = gie; ha.lens = lens; ha.S = S;
  for (int t = 0; t < 32; ++t) {
    gru_step(d->gru, t == 0 ? c.w(d->init_input) : tok_t, t == 0 ? 0 : 2 * PN_HE, 2 * PN_HE, ldt, ht, t & 1, PN_HT, gi_z, nullptr, 0);
    // decode_notes: initial hidden of the notes GRU, and the notes_summary part of its input (constant over the slots)
    const size_t ht_out = (size_t)((t + 1) & 1) * R * PN_HT;
    c.launch(PF_K_SMALL, 0.0, [&] { return launch_linear(ht + ht_out, PN_HT, c.w(d->t2n.w), PN_HT, c.w(d->t2n.b), hn, PN_HN, R, PN_HN, PN_HT, c.s); });
    c.launch(PF_K_SMALL, 0.0, [&] { return launch_linear(ht + ht_out, PN_HT, c.w(d->notes_gru.w_ih), ldn, c.w(d->notes_gru.b_ih), gi_ns, 3 * PN_HN, R, 3 * PN_HN, PN_HT, c.s); });
    for (int sl = 1; sl < S; ++sl) {
      gru_step(d->notes_gru, nullptr, 0, 0, 0, hn, (sl - 1) & 1, PN_HN, gi_ns, sl == 1 ? c.w(d->tn_sos) : gi_tok, sl == 1 ? 0 : 3 * PN_HN);
      c.launch(PF_K_SMALL, 0.0, [&] {
        ha.h = hn + (size_t)(sl & 1) * R * PN_HN; ha.t = t; ha.s = sl;
        if (d->HD == 64) hipLaunchKernelGGL(pnotree_heads_kernel<64>, dim3(R), dim3(256), 0, c.s, ha);
        else hipLaunchKernelGGL(pnotree_heads_kernel<16>, dim3(R), dim3(256), 0, c.s, ha);
        return launched();
      });
    }
    if (t == 31) break;
    c.launch(PF_K_SMALL, 0.0, [&] {
      hipLaunchKernelGGL(pnotree_emb_gru_kernel, dim3(R, 2), dim3(3 * PN_HE), 0, c.s, (const float*)gie, c.w(d->te_sos), c.w(d->whh_t),
                         c.w(d->emb_gru[0].b_hh), c.w(d->emb_gru[1].b_hh), (const int*)lens, tok_t, S);
      return launched();
    });
  }
  return c.rc;
}

PlanSize dec_plan(const pf_decoder* d, int rows) {
  PlanCtx c;
  c.B = rows;
  return plan_sizes(c, [d](PlanCtx& dry) { dec_run(d, dry, nullptr, nullptr, nullptr, nullptr, nullptr); });
}
// the forced chord walk with every step fed back (mask 0): the most launches any mask enqueues; the workspace is the greedy walk's
PlanSize dec_plan_forced(const pf_decoder* d, int rows, int feedback) {
  PlanCtx c;
  c.B = rows;
  const ChordForce f{nullptr, 0, feedback};
  return plan_sizes(c, [d, &f](PlanCtx& dry) { dec_run(d, dry, nullptr, nullptr, nullptr, nullptr, nullptr, &f); });
}

}  // namespace

extern "C" {

int pf_decoder_create(int kind, int max_simu_note, int input_dim, int z_input_dim, int hidden_dim, int z_dim, int n_step,
                      pf_decoder** out) {
  PF_REQUIRE(out && (kind == PF_DEC_CHORD || kind == PF_DEC_PNOTREE), "pf_decoder_create: bad kind");
  std::unique_ptr<pf_decoder> d(new pf_decoder());
  d->kind = kind;
  WeightTable& wt = d->wt;
  if (kind == PF_DEC_PNOTREE) {   // dl_modules/pianotree_dec.py:11-99, default sizes; hidden_dim = dec_dur_hid_size (0: the default 16)
    PF_REQUIRE(max_simu_note >= 2 && max_simu_note <= 32, "pf_decoder_create: max_simu_note must be in 2..32");
    PF_REQUIRE(hidden_dim == 0 || hidden_dim == 16 || hidden_dim == 64, "pf_decoder_create: dec_dur_hid_size (hidden_dim) must be 16 or 64, got %d", hidden_dim);
    d->S = max_simu_note;
    d->HD = hidden_dim ? hidden_dim : 16;
    const int PN_HD = d->HD;
    d->init_input = wt.raw("dec_init_input", {2 * PN_HE});
    d->dur_sos = wt.raw("dur_sos_token", {PN_DW});
    d->note_emb = wt.linear("note_embedding", PN_E, PN_TOK);
    d->z2hid = wt.linear("z2dec_hid_linear", PN_HT, PN_Z);
    d->z2in = wt.linear("z2dec_in_linear", PN_ZIN, PN_Z);
    wt.gru("dec_notes_emb_gru", PN_E, PN_HE, 2, d->emb_gru);
    wt.gru("dec_time_gru", PN_ZIN + 2 * PN_HE, PN_HT, 1, &d->gru);
    d->t2n = wt.linear("dec_time_to_notes_hid", PN_HN, PN_HT);
    wt.gru("dec_notes_gru", PN_HT + PN_E, PN_HN, 1, &d->notes_gru);
    d->pitch = wt.linear("pitch_out_linear", PN_P, PN_HN);
    wt.gru("dec_dur_gru", PN_DW, PN_HD, 1, &d->dur_gru);
    d->dur_hid = wt.linear("dur_hid_linear", PN_HD, PN_P + PN_HN);
    d->dur_out = wt.linear("dur_out_linear", 2, PN_HD);
    d->tn = wt.alloc((size_t)PN_TROWS * 3 * PN_HN);
    d->te = wt.alloc((size_t)PN_TROWS * 6 * PN_HE);
    d->tn_sos = wt.alloc(3 * PN_HN);
    d->te_sos = wt.alloc(6 * PN_HE);
    d->whh_t = wt.alloc((size_t)2 * PN_HE * 3 * PN_HE);
    if (d->HD == 64) d->wdhh_t = wt.alloc((size_t)64 * 3 * 64);
  } else {                        // dl_modules/chord_dec.py:8-25
    PF_REQUIRE(input_dim == 36, "pf_decoder_create: the chord token is root 12 | chroma 12 | bass 12 (input_dim 36)");
    PF_REQUIRE(z_input_dim > 0 && z_dim > 0 && n_step > 0, "pf_decoder_create: bad dims");
    PF_REQUIRE(hidden_dim > 0 && hidden_dim % 4 == 0 && hidden_dim <= 1024, "pf_decoder_create: hidden_dim must be a multiple of 4, at most 1024");
    PF_REQUIRE(z_dim <= 2048 && z_input_dim <= 2048, "pf_decoder_create: z_dim / z_input_dim at most 2048");
    d->input_dim = input_dim; d->z_input_dim = z_input_dim; d->hidden = hidden_dim; d->z_dim = z_dim; d->n_step = n_step;
    d->init_input = wt.raw("init_input", {36});
    d->z2hid = wt.linear("z2dec_hid", hidden_dim, z_dim);
    d->z2in = wt.linear("z2dec_in", z_input_dim, z_dim);
    wt.gru("gru", input_dim + z_input_dim, hidden_dim, 1, &d->gru);
    d->root = wt.linear("root_out", 12, hidden_dim);
    d->chroma = wt.linear("chroma_out", 24, hidden_dim);
    d->bass = wt.linear("bass_out", 12, hidden_dim);
  }
  *out = d.release();
  return PF_OK;
}

void pf_decoder_destroy(pf_decoder* d) { delete d; }
size_t pf_decoder_weight_bytes(const pf_decoder* d) { return d ? d->wt.blob_floats * sizeof(float) : 0; }
int pf_decoder_n_params(const pf_decoder* d) { return d ? (int)d->wt.params.size() : 0; }
int pf_decoder_param_info(const pf_decoder* d, int i, char* key_buf, size_t key_buf_len, int64_t shape[4], int* ndim) {
  PF_REQUIRE(d, "pf_decoder_param_info: null argument");
  return d->wt.param_info("pf_decoder_param_info", i, key_buf, key_buf_len, shape, ndim);
}
int pf_decoder_pack_param(pf_decoder* d, const char* key, const float* src, const int64_t* shape, int ndim, void* host_blob) {
  PF_REQUIRE(d, "pf_decoder_pack_param: null argument");
  return d->wt.pack_param("pf_decoder_pack_param", "decoder", key, src, shape, ndim, host_blob);
}
int pf_decoder_pack_missing(const pf_decoder* d, char* buf, size_t buf_len) { return d ? d->wt.pack_missing(buf, buf_len) : set_error(PF_EINVAL, "null handle"); }

// The PianoTree blob ends in a region the packing leaves empty: bind fills it on the device (token tables, start-token rows, the
// transposed W_hh of the embedding GRU) and waits for that, so the blob must be writable and 16-byte aligned.
int pf_decoder_bind_weights(pf_decoder* d, void* dev_blob) {
  PF_REQUIRE(d && dev_blob, "pf_decoder_bind_weights: null argument");
  PF_REQUIRE(((uintptr_t)dev_blob & 15) == 0, "pf_decoder_bind_weights: the blob must be 16-byte aligned");
  int rc = d->wt.bind("pf_decoder_bind_weights", dev_blob, false);
  if (rc || d->kind != PF_DEC_PNOTREE) return rc;
  float* W = (float*)dev_blob;
  PF_CHECK_HIP(hipDeviceSynchronize());   // the copy that brought the blob may be on any stream
  const float *ew = W + d->note_emb.w, *eb = W + d->note_emb.b;
  hipStream_t s = nullptr;
  hipLaunchKernelGGL(token_table_kernel, dim3(cdiv(3 * PN_HN, 128), PN_TROWS), dim3(128), 0, s, W + d->notes_gru.w_ih, PN_HT + PN_E, PN_HT,
                     3 * PN_HN, ew, eb, (const float*)nullptr, W + d->tn, 3 * PN_HN, 0);
  for (int dir = 0; dir < 2; ++dir) {
    const GruOff& g = d->emb_gru[dir];
    hipLaunchKernelGGL(token_table_kernel, dim3(cdiv(3 * PN_HE, 128), PN_TROWS), dim3(128), 0, s, W + g.w_ih, PN_E, 0, 3 * PN_HE, ew, eb,
                       W + g.b_ih, W + d->te, 6 * PN_HE, dir * 3 * PN_HE);
    hipLaunchKernelGGL(transpose_kernel, dim3(cdiv(3 * PN_HE * PN_HE, 256)), dim3(256), 0, s, W + g.w_hh, 3 * PN_HE, PN_HE,
                       W + d->whh_t + (size_t)dir * PN_HE * 3 * PN_HE);
  }
  if (d->HD == 64)
    hipLaunchKernelGGL(transpose_kernel, dim3(cdiv(3 * 64 * 64, 256)), dim3(256), 0, s, W + d->dur_gru.w_hh, 3 * 64, 64, W + d->wdhh_t);
  hipLaunchKernelGGL(sos_row_kernel, dim3(cdiv(3 * PN_HN, 128)), dim3(128), 0, s, W + d->tn, 3 * PN_HN, W + d->tn_sos);
  hipLaunchKernelGGL(sos_row_kernel, dim3(cdiv(6 * PN_HE, 128)), dim3(128), 0, s, W + d->te, 6 * PN_HE, W + d->te_sos);
  PF_CHECK_HIP(hipGetLastError());
  PF_CHECK_HIP(hipDeviceSynchronize());
  return PF_OK;
}

size_t pf_decoder_workspace_bytes(const pf_decoder* d, int rows) { return (d && rows > 0) ? dec_plan(d, rows).bytes() : 0; }
int pf_decoder_launches(const pf_decoder* d, int rows) { return (d && rows > 0) ? dec_plan(d, rows).n_launch : 0; }

int pf_decoder_forward(pf_decoder* d, const float* z, int rows, float* out0, float* out1, float* out2, int32_t* est, void* workspace,
                       size_t workspace_bytes, void* stream) {
  PF_REQUIRE(d && z && out0 && out1 && workspace && rows > 0, "pf_decoder_forward: bad arguments");
  if (!d->wt.wdev) return set_error(PF_ESTATE, "pf_decoder_forward: weights not bound");
  PF_REQUIRE(d->kind != PF_DEC_CHORD || out2, "pf_decoder_forward: the chord decoder writes three outputs");
  PF_REQUIRE(d->kind != PF_DEC_PNOTREE || est, "pf_decoder_forward: the PianoTree decoder writes the integer grid");
  PlanCtx c;
  c.B = rows;
  const int rc = c.use_workspace("pf_decoder_forward", workspace, workspace_bytes, dec_plan(d, rows), stream, d->wt.wdev, 16);
  if (rc != PF_OK) return rc;
  return dec_run(d, c, z, out0, out1, out2, est);
}

static bool chord_handle(const pf_decoder* d) { return d && d->kind == PF_DEC_CHORD; }
static bool feedback_known(int f) { return f == PF_FEEDBACK_ROW || f == PF_FEEDBACK_BATCH; }
size_t pf_decoder_forced_workspace_bytes(const pf_decoder* d, int rows) {
  return (chord_handle(d) && rows > 0) ? dec_plan_forced(d, rows, PF_FEEDBACK_ROW).bytes() : 0;
}
int pf_decoder_forced_launches(const pf_decoder* d, int rows, int feedback) {
  return (chord_handle(d) && rows > 0 && feedback_known(feedback)) ? dec_plan_forced(d, rows, feedback).n_launch : 0;
}

int pf_decoder_forward_forced(pf_decoder* d, const pf_chord_forced_args* a, void* stream) {
  PF_REQUIRE(d && a, "pf_decoder_forward_forced: null argument");
  PF_REQUIRE(d->kind == PF_DEC_CHORD, "pf_decoder_forward_forced: teacher forcing is built for the chord decoder only");
  PF_REQUIRE(d->n_step - 1 <= 64, "pf_decoder_forward_forced: force_mask holds 64 steps, n_step - 1 = %d", d->n_step - 1);
  PF_REQUIRE(a->gt, "pf_decoder_forward_forced: gt (the chord matrix [rows][n_step][36]) is null");
  PF_REQUIRE(feedback_known(a->feedback), "pf_decoder_forward_forced: unknown feedback %d (PF_FEEDBACK_ROW or PF_FEEDBACK_BATCH)", a->feedback);
  PF_REQUIRE(a->z && a->root && a->chroma && a->bass && a->workspace && a->rows > 0, "pf_decoder_forward_forced: bad arguments");
  PlanCtx c;
  c.B = a->rows;
  const int rc = c.use_workspace("pf_decoder_forward_forced", a->workspace, a->workspace_bytes, dec_plan_forced(d, a->rows, a->feedback), stream,
                                 d->wt.wdev, 16);
  if (rc != PF_OK) return rc;
  if (!d->wt.wdev) return set_error(PF_ESTATE, "pf_decoder_forward_forced: weights not bound");
  const ChordForce f{a->gt, a->force_mask, a->feedback};
  return dec_run(d, c, a->z, a->root, a->chroma, a->bass, nullptr, &f);
}

}  // extern "C"
