// chordrec.hip - chord recognition of generated rolls (include/pfhip.h, pf_chord_recognize; DESIGN.md 3, "Chord recognition").
// One workgroup per song, four phases separated by workgroup barriers:
//   1. features   a wave owns whole images (a note never crosses an image end, so images are independent).  Lane l is key l and key
//                 64 + l; it walks the image's steps a beat at a time, keeping "a note is open on this key" and the length of its stretch
//                 inside the beat.  The per-class maximum and the per-step lowest key come out of ballots: integers, order-free.
//   2. prefix     24 threads turn the per-beat tables into running sums in place, so that a window sum is one subtraction.
//   3. scores     a wave owns a window (i, j); lane l scores classes l, l + 64, ... (their constants live in registers for the whole
//                 phase) in float64 in the reference's operation order and keeps its first maximum; a butterfly picks the wave's.
//   4. decode     thread 0 runs the dynamic programme and the backtrack over the per-window bests held in LDS (at most 5 per beat);
//                 labels, rows and the comparison counters are then written by all threads.
#include "pf_internal.h"

namespace pf {

constexpr int kCrMaxWaves = 16;
constexpr int kCrWin = 5;                                    // windows per beat: decode() breaks one beat past a downbeat, so j <= 4
constexpr int kCrPerLane = PF_CHORDREC_MAX_CLASSES / 64;     // 9 classes per lane

struct CrShared {
  double best[PF_CHORDREC_MAX_BEATS * kCrWin];              // best obs of window (i, j) at [i * 5 + j]
  double dp[PF_CHORDREC_MAX_BEATS];
  int32_t part[kCrMaxWaves][PF_CHORDREC_NCOUNT];
  int16_t pc[(PF_CHORDREC_MAX_BEATS + 1) * 12];             // row j + 1: chroma_q of beat j, then the running sum up to and including it
  int16_t pb[(PF_CHORDREC_MAX_BEATS + 1) * 12];             // the same for bass_q
  int16_t bcls[PF_CHORDREC_MAX_BEATS * kCrWin];             // class of best[]
  int16_t prec[PF_CHORDREC_MAX_BEATS], prei[PF_CHORDREC_MAX_BEATS];
  int16_t lab[PF_CHORDREC_MAX_BEATS];                       // label | 0x4000 on the first beat of a recognised segment
  int32_t nseg;
};

// arg-max of twelve floats, ties (and a NaN, which never compares greater) to the lowest index; *any: some entry is > 0.5
__device__ __forceinline__ int cr_argmax12(const float* __restrict__ v, bool* any) {
  float best = v[0];
  int bi = 0;
  bool pos = best > 0.5f;
  for (int i = 1; i < 12; ++i) {
    const float c = v[i];
    pos = pos || c > 0.5f;
    if (c > best) { best = c; bi = i; }
  }
  *any = pos;
  return bi;
}
__device__ __forceinline__ unsigned cr_bits12(const float* __restrict__ v) {
  unsigned m = 0;
  for (int i = 0; i < 12; ++i) m |= (v[i] > 0.5f) ? (1u << i) : 0u;
  return m;
}

__global__ __launch_bounds__(64 * kCrMaxWaves) void chord_recognize_kernel(pf_chord_recognize_args a) {
  __shared__ CrShared sh;
  const int song = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
  const int steps = a.steps, beats_img = steps >> 2, beats = a.segments * beats_img;
  int32_t* chroma_q = a.chroma_q + (size_t)song * beats * 12;
  int32_t* bass_q = a.bass_q + (size_t)song * beats * 12;

  // ---------------------------------------------------------------- 1. features
  constexpr unsigned long long kClass0 = 0x1001001001001001ull;                 // keys 0, 12, ..., 60
  // the keys of class k among the lower 64 are bits k, k + 12, ...; among the upper 64 (key = 64 + bit, 64 % 12 == 4) those of (k + 8) % 12
  const unsigned long long cm[2] = {lane < 12 ? kClass0 << lane : 0ull, lane < 12 ? kClass0 << ((lane + 8) % 12) : 0ull};
  if (tid < 12) sh.pc[tid] = 0, sh.pb[tid] = 0;
  for (int g = wave; g < a.segments; g += nwaves) {
    const float* on = a.prmat2c + ((size_t)song * a.segments + g) * 2 * steps * 128;
    const float* su = on + (size_t)steps * 128;
    bool open[2] = {false, false};                                              // a note sounds on this lane's key (closed at the image start)
    for (int jb = 0; jb < beats_img; ++jb) {
      float o[4][2], s[4][2];
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const size_t i = (size_t)(4 * jb + k) * 128 + 64 * h + lane;
          o[k][h] = on[i];
          s[k][h] = su[i];
        }
      int cur[2] = {0, 0}, longest[2] = {0, 0}, bass = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        unsigned long long snd[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const bool is_on = a.custom_round ? (o[k][h] > 0.95f && o[k][h] < 1.05f) : (o[k][h] > 0.5f);
          if (!(s[k][h] > 0.5f)) { open[h] = false; cur[h] = 0; }              // the note-off: every open note of the key ends here
          open[h] = open[h] || is_on;
          if (open[h]) longest[h] = max(longest[h], ++cur[h]);
          snd[h] = __ballot(open[h]);
        }
        const int low = snd[0] ? __builtin_ctzll(snd[0]) : snd[1] ? 64 + __builtin_ctzll(snd[1]) : -1;
        bass += (low >= 0 && low % 12 == lane) ? 2 : 0;                         // two half-step sub-beats of an eighth each
      }
      int cmax = 0;
#pragma unroll
      for (int v = 1; v <= 4; ++v) {
        const unsigned long long m0 = __ballot(longest[0] >= v), m1 = __ballot(longest[1] >= v);
        if ((m0 & cm[0]) | (m1 & cm[1])) cmax = v;
      }
      if (lane < 12) {
        const int j = g * beats_img + jb;
        sh.pc[(j + 1) * 12 + lane] = (int16_t)cmax;
        sh.pb[(j + 1) * 12 + lane] = (int16_t)bass;
        chroma_q[(size_t)j * 12 + lane] = cmax;
        bass_q[(size_t)j * 12 + lane] = bass;
      }
    }
  }
  __syncthreads();

  // ---------------------------------------------------------------- 2. running sums (at most 4 * 512 and 8 * 512: they fit 16 bits)
  if (tid < 24) {
    int16_t* p = (tid < 12 ? sh.pc : sh.pb) + tid % 12;
    int run = 0;
    for (int j = 1; j <= beats; ++j) {
      run += p[j * 12];
      p[j * 12] = (int16_t)run;
    }
  }
  __syncthreads();

  // ---------------------------------------------------------------- 3. the best class of every window
  {
    int bits[kCrPerLane];
    double csize[kCrPerLane], cslash[kCrPerLane];
#pragma unroll
    for (int k = 0; k < kCrPerLane; ++k) {
      const int c = lane + 64 * k;
      const bool ok = c < a.n_classes;
      bits[k] = ok ? a.cls_bits[c] : -1;                                        // -1: no such class
      csize[k] = ok ? a.cls_const[2 * c] : 0.0;
      cslash[k] = ok ? a.cls_const[2 * c + 1] : 0.0;
    }
    const double c_half = a.consts[12], c_even = a.consts[13], c_none = a.consts[14];
    for (int p = wave; p < beats * kCrWin; p += nwaves) {
      const int i = p / kCrWin, j = p % kCrWin;
      if (j > i || j > (i & 3) + 1) continue;                                   // before the song, or past decode()'s break
      const int first = i - j;                                                  // the window is beats first .. i
      int wc[12], total = 0;
#pragma unroll
      for (int k = 0; k < 12; ++k) {
        wc[k] = sh.pc[(i + 1) * 12 + k] - sh.pc[first * 12 + k];
        total += wc[k];
      }
      const double bonus_j = a.consts[j];
      const double bonus_half = (first & 3) == 2 ? c_half : 0.0, bonus_even = (first & 1) == 0 ? c_even : 0.0;
      double best = 0.0;
      int bcls = -1;
#pragma unroll
      for (int k = 0; k < kCrPerLane; ++k) {
        if (bits[k] < 0) continue;
        const int size = (bits[k] >> 16) & 15, bass_cls = (bits[k] >> 12) & 15;
        double score = c_none;
        if (size > 0) {
          int in = 0;
#pragma unroll
          for (int q = 0; q < 12; ++q) in += ((bits[k] >> q) & 1) ? wc[q] : 0;
          const int wb = bass_cls < 12 ? sh.pb[(i + 1) * 12 + bass_cls] - sh.pb[first * 12 + bass_cls] : 0;
          const double num = (double)(2 * in - total) * 0.25;                   // exact
          score = ((num / (double)size + 0.5 * ((double)wb * 0.125)) - csize[k]) - cslash[k];
        }
        const double obs = ((score + bonus_j) + bonus_half) + bonus_even;
        if (bcls < 0 || obs > best) { best = obs; bcls = lane + 64 * k; }       // ascending classes: the first maximum stays
      }
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const double ob = __shfl_xor(best, d);
        const int oc = __shfl_xor(bcls, d);
        if (oc >= 0 && (bcls < 0 || ob > best || (ob == best && oc < bcls))) { best = ob; bcls = oc; }
      }
      if (lane == 0) {
        sh.best[p] = best;
        sh.bcls[p] = (int16_t)bcls;
      }
    }
  }
  __syncthreads();

  // ---------------------------------------------------------------- 4. decode: the serial tail
  if (tid == 0) {
    for (int i = 0; i < beats; ++i) {
      double d = -INFINITY;
      int pcls = 0, pidx = 0;
      const int jmax = min(i, (i & 3) + 1);
      for (int j = 0; j <= jmax; ++j) {
        const double cand = (i - j == 0 ? 0.0 : sh.dp[i - j - 1]) + sh.best[i * kCrWin + j];
        if (d < cand) { d = cand; pcls = sh.bcls[i * kCrWin + j]; pidx = i - j - 1; }
      }
      sh.dp[i] = d;
      sh.prec[i] = (int16_t)pcls;
      sh.prei[i] = (int16_t)pidx;
    }
    int nseg = 0;
    for (int cur = beats - 1; cur >= 0;) {
      const int prev = sh.prei[cur], cls = sh.prec[cur];
      for (int b = prev + 1; b <= cur; ++b) sh.lab[b] = (int16_t)(cls | (b == prev + 1 ? 0x4000 : 0));
      cur = prev;
      ++nseg;
    }
    sh.nseg = nseg;
    a.path_score[song] = sh.dp[beats - 1];
  }
  __syncthreads();

  int cnt[PF_CHORDREC_NCOUNT] = {0};
  for (int b = tid; b < beats; b += blockDim.x) {
    const int label = sh.lab[b] & 0x3fff;
    a.labels[(size_t)song * beats + b] = label;
    a.bounds[(size_t)song * beats + b] = (sh.lab[b] >> 14) & 1;
    if (a.chord) {
      const float* r = a.cls_rows + (size_t)label * 36;
      const float* c = a.chord + ((size_t)song * beats + b) * 36;
      bool r_has, c_has, rb_has, cb_has;
      const int r_root = cr_argmax12(r, &r_has), c_root = cr_argmax12(c, &c_has);
      const int r_bass = cr_argmax12(r + 24, &rb_has);
      int c_bass = cr_argmax12(c + 24, &cb_has);
      if (a.bass_relative) c_bass = (c_bass + c_root) % 12;
      const unsigned rm = cr_bits12(r + 12), cmask = cr_bits12(c + 12);
      const bool root = r_root == c_root && r_has == c_has, chroma = rm == cmask, bass = r_bass == c_bass && rb_has == cb_has;
      cnt[PF_CHORDREC_ROOT_HIT] += root;
      cnt[PF_CHORDREC_CHROMA_HIT] += chroma;
      cnt[PF_CHORDREC_BASS_HIT] += bass;
      cnt[PF_CHORDREC_FULL_HIT] += root && chroma && bass;
      cnt[PF_CHORDREC_CHROMA_INTER] += __popc(rm & cmask);
      cnt[PF_CHORDREC_CHROMA_UNION] += __popc(rm | cmask);
    }
  }
  for (int e = tid; e < beats * 36; e += blockDim.x)
    a.rows[(size_t)song * beats * 36 + e] = a.cls_rows[(size_t)(sh.lab[e / 36] & 0x3fff) * 36 + e % 36];
#pragma unroll
  for (int c = 0; c < PF_CHORDREC_NCOUNT; ++c) {
    int v = cnt[c];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
    if (lane == 0) sh.part[wave][c] = v;
  }
  __syncthreads();
  if (tid < PF_CHORDREC_NCOUNT) {
    int v = 0;
    for (int w = 0; w < nwaves; ++w) v += sh.part[w][tid];
    if (tid == PF_CHORDREC_BEATS) v = beats;
    if (tid == PF_CHORDREC_SEGMENTS) v = sh.nseg;
    a.counters[(size_t)song * PF_CHORDREC_NCOUNT + tid] = v;
  }
}

int launch_chord_recognize(const pf_chord_recognize_args& a, hipStream_t stream) {
  PF_REQUIRE(a.prmat2c && a.songs > 0 && a.segments > 0 && a.steps > 0, "chord_recognize: bad arguments (prmat2c %p, songs = %d, segments = %d, steps = %d)",
             (const void*)a.prmat2c, a.songs, a.segments, a.steps);
  PF_REQUIRE(a.steps % 16 == 0, "chord_recognize: steps = %d is not a whole number of bars (16 steps each)", a.steps);
  PF_REQUIRE((long long)a.segments * (a.steps / 4) <= PF_CHORDREC_MAX_BEATS, "chord_recognize: %d segments of %d steps are more than %d beats per song",
             a.segments, a.steps, PF_CHORDREC_MAX_BEATS);
  PF_REQUIRE(a.cls_bits && a.cls_const && a.cls_rows && a.consts, "chord_recognize: null vocabulary table (cls_bits %p, cls_const %p, cls_rows %p, consts %p)",
             (const void*)a.cls_bits, (const void*)a.cls_const, (const void*)a.cls_rows, (const void*)a.consts);
  PF_REQUIRE(a.n_classes >= 1 && a.n_classes <= PF_CHORDREC_MAX_CLASSES, "chord_recognize: n_classes = %d outside 1..%d", a.n_classes,
             PF_CHORDREC_MAX_CLASSES);
  PF_REQUIRE(a.max_template >= 1 && a.max_template <= 12, "chord_recognize: max_template = %d outside 1..12", a.max_template);
  PF_REQUIRE(a.labels && a.bounds && a.rows && a.counters && a.path_score && a.chroma_q && a.bass_q,
             "chord_recognize: null output (labels %p, bounds %p, rows %p, counters %p, path_score %p, chroma_q %p, bass_q %p)", (void*)a.labels,
             (void*)a.bounds, (void*)a.rows, (void*)a.counters, (void*)a.path_score, (void*)a.chroma_q, (void*)a.bass_q);
  const uintptr_t a4 = (uintptr_t)a.prmat2c | (uintptr_t)a.chord | (uintptr_t)a.cls_bits | (uintptr_t)a.cls_rows | (uintptr_t)a.labels |
                       (uintptr_t)a.bounds | (uintptr_t)a.rows | (uintptr_t)a.counters | (uintptr_t)a.chroma_q | (uintptr_t)a.bass_q;
  const uintptr_t a8 = (uintptr_t)a.cls_const | (uintptr_t)a.consts | (uintptr_t)a.path_score;
  PF_REQUIRE(a4 % 4 == 0 && a8 % 8 == 0, "chord_recognize: pointers must be 4-byte aligned (cls_const, consts, path_score: 8-byte)");
  const int beats = a.segments * (a.steps / 4);
  const int waves = min(kCrMaxWaves, cdiv(beats * kCrWin, 4));
  hipLaunchKernelGGL(chord_recognize_kernel, dim3(a.songs), dim3(64 * waves), 0, stream, a);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}

}  // namespace pf
