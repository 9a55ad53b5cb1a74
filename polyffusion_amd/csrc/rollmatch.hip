// rollmatch.hip - packed piano rolls and their nearest neighbours under transposition (include/pfhip.h, pf_roll_pack / pf_roll_match;
// DESIGN.md 3, "Roll matching").  Integer work only: compares, AND, popcount, int64 cross-multiplication.  No atomics, no floating point.
//
//   pack     a wave per row of 128 keys: lane l holds key l and key 64 + l of both channels, two ballots per plane are the row's four words.
//   counts   |qs| of every (query, shift): the query row ANDed with the shifted all-ones row, so that notes leaving the keyboard are dropped.
//   match    a bit-GEMM.  A workgroup owns PF_ROLL_MATCH_CHUNK corpus windows (one per thread) and kQT queries.  Shifting the query by s
//            and ANDing with the window equals ANDing the query with the window shifted the other way - on bit indices,
//            sum_j q[j + s] c[j] = sum_i q[i] c[i - s] - so the thread shifts its own corpus row (4 funnel shifts, in registers) once per
//            (shift, step) and meets all kQT query rows with it: 8 lane-ops (v_and + accumulating v_bcnt) per word quadruple and query.
//            The query rows are the same for every thread: they lie in LDS and are read as broadcasts.  Per query the thread keeps the
//            best shift of its window (ties to the lowest k); the chunk's top-k per query is then chosen by one wave per query from LDS
//            and written to the workspace as a partial list.
//   merge    a wave per query walks the partial lists in chunk order and picks the top-k.
// Selection never marks anything as taken: candidates are totally ordered (fraction descending, then index ascending, indices unique),
// so round r picks the best candidate strictly after the winner of round r - 1.
#include "pf_internal.h"

namespace pf {

constexpr int kQT = 4;                          // queries per workgroup of the match kernel (accumulators per thread)
constexpr int kChunk = PF_ROLL_MATCH_CHUNK;     // corpus windows per workgroup, one per thread
constexpr int kCntStride = 32;                  // ints per query in the |qs| table (2 * 15 + 1 shifts, padded)
static_assert(kChunk == 256, "the selection below deals four candidates to each of 64 lanes");

__device__ __forceinline__ bool rm_round(float v, int custom) { return custom ? (v > 0.95f && v < 1.05f) : (v > 0.5f); }
__device__ __forceinline__ int rm_shift_of(int k) { return (k & 1) ? -((k + 1) >> 1) : (k >> 1); }      // 0, -1, +1, -2, +2, ...
// bit j of the result is bit j - s of c (zero where j - s leaves 0..127); |s| <= 15
__device__ __forceinline__ uint4 rm_shift128(uint4 c, int s) {
  uint4 r;
  if (s >= 0) {
    auto up = [s](uint32_t hi, uint32_t lo) { return (uint32_t)(((((uint64_t)hi << 32) | lo) << s) >> 32); };
    r.x = c.x << s;
    r.y = up(c.y, c.x);
    r.z = up(c.z, c.y);
    r.w = up(c.w, c.z);
  } else {
    const int d = -s;
    auto down = [d](uint32_t hi, uint32_t lo) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> d); };
    r.x = down(c.y, c.x);
    r.y = down(c.z, c.y);
    r.z = down(c.w, c.z);
    r.w = c.w >> d;
  }
  return r;
}

// ------------------------------------------------------------------ pack
__global__ __launch_bounds__(256) void roll_pack_kernel(const float* __restrict__ x, long long rows, int steps, int custom,
                                                        uint32_t* __restrict__ bits) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;                                                      // wave-uniform
  const long long img = row / steps, t = row % steps;
  const float* on = x + ((img * 2) * steps + t) * 128;
  const float* su = on + (long long)steps * 128;
  const bool o0 = rm_round(on[lane], custom), o1 = rm_round(on[64 + lane], custom);
  const bool s0 = o0 || rm_round(su[lane], custom), s1 = o1 || rm_round(su[64 + lane], custom);
  const unsigned long long w[4] = {__ballot(o0), __ballot(o1), __ballot(s0), __ballot(s1)};
  if (lane < 8) {                                                               // lane = plane * 4 + word
    const unsigned long long v = w[lane >> 1];
    bits[((long long)(lane >> 2) * rows + row) * 4 + (lane & 3)] = (uint32_t)((lane & 1) ? v >> 32 : v);
  }
}

int launch_roll_pack(const float* x, int n, int steps, int custom_round, uint32_t* bits, hipStream_t stream) {
  PF_REQUIRE(x && bits, "roll_pack: null pointer (prmat2c %p, bits %p)", (const void*)x, (void*)bits);
  PF_REQUIRE(n > 0 && steps > 0, "roll_pack: bad shape (n = %d, steps = %d)", n, steps);
  PF_REQUIRE(((uintptr_t)x | (uintptr_t)bits) % 4 == 0, "roll_pack: pointers must be 4-byte aligned");
  const long long rows = (long long)n * steps;
  PF_REQUIRE((rows + 3) / 4 <= 0x7fffffffLL, "roll_pack: %lld rows are more than one launch takes", rows);
  hipLaunchKernelGGL(roll_pack_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, x, rows, steps, custom_round != 0, bits);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}

// ------------------------------------------------------------------ |qs| per (query, shift)
__global__ __launch_bounds__(64) void roll_match_counts_kernel(const uint32_t* __restrict__ a_bits, const int32_t* __restrict__ a_starts,
                                                               int steps, int nshift, int32_t* __restrict__ qcnt) {
  const int q = blockIdx.x, k = threadIdx.x;
  if (k >= kCntStride) return;
  int n = 0;
  if (k < nshift) {
    const uint4 m = rm_shift128(make_uint4(~0u, ~0u, ~0u, ~0u), rm_shift_of(k));
    const uint4* row = reinterpret_cast<const uint4*>(a_bits + (long long)a_starts[q] * 4);
    for (int t = 0; t < steps; ++t) {
      const uint4 v = row[t];
      n += __popc(v.x & m.x) + __popc(v.y & m.y) + __popc(v.z & m.z) + __popc(v.w & m.w);
    }
  }
  qcnt[q * kCntStride + k] = n;
}

// ------------------------------------------------------------------ selection
struct RmCand {
  int inter, uni, idx;       // inter < 0: no candidate (loses to everything)
};
// a comes strictly before b in the order "fraction descending, index ascending"; a union of 0 counts as 0 / 1
__device__ __forceinline__ bool rm_before(const RmCand& a, const RmCand& b) {
  const long long l = (long long)a.inter * max(b.uni, 1), r = (long long)b.inter * max(a.uni, 1);
  return l > r || (l == r && a.idx < b.idx);
}
__device__ __forceinline__ RmCand rm_wave_first(RmCand c) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    RmCand o;
    o.inter = __shfl_xor(c.inter, d);
    o.uni = __shfl_xor(c.uni, d);
    o.idx = __shfl_xor(c.idx, d);
    if (rm_before(o, c)) c = o;
  }
  return c;
}
constexpr int kNoIdx = 0x7fffffff;

// ------------------------------------------------------------------ match
struct RmMatch {
  const uint32_t* a_bits;
  const int32_t* a_starts;
  const uint32_t* b_bits;
  const int32_t* b_starts;
  const int32_t* qcnt;
  int32_t* part;             // [na][nchunks][topk][4]: index, shift, inter, union
  int32_t *tab_inter, *tab_union, *tab_shift;
  int na, nb, steps, nshift, topk, nchunks;
};

// acc + popcount(x): the accumulating form of v_bcnt_u32_b32, one lane-op (the compiler prefers a bare count and a three-way add)
__device__ __forceinline__ int rm_bcnt(uint32_t x, int acc) {
  int r;
  asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
  return r;
}
// One pass over the window's rows for one shift: acc[i] += |shifted row AND row of query i|.  DIR is the sign of s, so that the loop
// holds no branch on it; DIR == 0 also counts the window's own cells.
// The corpus side: a thread reads its own window, so a wave's load touches 64 different cache lines.  It therefore takes kBlock = 8 rows,
// one whole 128-byte line's worth, in eight back-to-back loads, one block ahead of their use: every line is fetched once per pass instead
// of once per row (measured: 0.93 ms against 1.03 ms per call of tools/bench_rollmatch.py).
// The query side: a tile of kTile rows of the kQT queries lies in LDS (8 KB); kRows rows of each are read at a time, every lane the same
// address (a broadcast ds_read_b128).  Reading the same rows through the scalar cache (the addresses are wave-uniform) measured the same.
// Rows past the end repeat the last row with the corpus side zeroed.
constexpr int kBlock = 8, kRows = 2, kTile = 128;
template <int DIR>
__device__ __forceinline__ void rm_scan(const uint4* __restrict__ cr, const uint4 (&qrow)[kQT][kTile], int steps, int s, int (&acc)[kQT],
                                        int& csize) {
  uint4 nxt[kBlock];
#pragma unroll
  for (int h = 0; h < kBlock; ++h) nxt[h] = cr[min(h, steps - 1)];
  for (int t0 = 0; t0 < steps; t0 += kBlock) {
    uint4 c[kBlock];
#pragma unroll
    for (int h = 0; h < kBlock; ++h) c[h] = t0 + h < steps ? nxt[h] : make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int h = 0; h < kBlock; ++h) nxt[h] = cr[min(t0 + kBlock + h, steps - 1)];
#pragma unroll
    for (int g = 0; g < kBlock; g += kRows) {
      if (t0 + g >= steps) break;                                              // wave-uniform
      uint4 q[kRows][kQT];
#pragma unroll
      for (int h = 0; h < kRows; ++h)
#pragma unroll
        for (int i = 0; i < kQT; ++i) q[h][i] = qrow[i][min(t0 + g + h, steps - 1)];
#pragma unroll
      for (int h = 0; h < kRows; ++h) {
        uint4 v = c[g + h];
        if (DIR == 0) {
          csize = rm_bcnt(v.x, csize);
          csize = rm_bcnt(v.y, csize);
          csize = rm_bcnt(v.z, csize);
          csize = rm_bcnt(v.w, csize);
        } else {
          v = rm_shift128(v, s);
        }
#pragma unroll
        for (int i = 0; i < kQT; ++i) {
          acc[i] = rm_bcnt(v.x & q[h][i].x, acc[i]);
          acc[i] = rm_bcnt(v.y & q[h][i].y, acc[i]);
          acc[i] = rm_bcnt(v.z & q[h][i].z, acc[i]);
          acc[i] = rm_bcnt(v.w & q[h][i].w, acc[i]);
        }
      }
    }
  }
}

__global__ __launch_bounds__(kChunk) void roll_match_kernel(RmMatch p) {
  __shared__ int32_t s_inter[kQT][kChunk], s_union[kQT][kChunk], s_shift[kQT][kChunk];
  __shared__ uint4 s_q[kQT][kTile];
  const int tid = threadIdx.x, chunk = blockIdx.x, q0 = blockIdx.y * kQT;
  const int b = chunk * kChunk + tid;
  const bool live = b < p.nb;
  const uint4* crow = reinterpret_cast<const uint4*>(p.b_bits + (long long)p.b_starts[live ? b : p.nb - 1] * 4);
  const uint4* qrow[kQT];
  int qi[kQT];
#pragma unroll
  for (int i = 0; i < kQT; ++i) {
    qi[i] = min(q0 + i, p.na - 1);                                              // a query past the end repeats the last one and is not written
    qrow[i] = reinterpret_cast<const uint4*>(p.a_bits + (long long)__builtin_amdgcn_readfirstlane(p.a_starts[qi[i]]) * 4);
  }
  int best_i[kQT] = {0}, best_u[kQT] = {0}, best_k[kQT] = {0}, csize = 0;
  for (int k = 0; k < p.nshift; ++k) {
    const int s = rm_shift_of(k);
    int acc[kQT];
#pragma unroll
    for (int i = 0; i < kQT; ++i) acc[i] = 0;
    for (int tile0 = 0; tile0 < p.steps; tile0 += kTile) {
      const int rows = min(kTile, p.steps - tile0);
      if (k == 0 || p.steps > kTile) {                                          // a window of one tile keeps it for every shift
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kQT; ++i)
          for (int t = tid; t < rows; t += kChunk) s_q[i][t] = qrow[i][tile0 + t];
        __syncthreads();
      }
      if (s == 0) rm_scan<0>(crow + tile0, s_q, rows, 0, acc, csize);
      else if (s > 0) rm_scan<1>(crow + tile0, s_q, rows, s, acc, csize);
      else rm_scan<-1>(crow + tile0, s_q, rows, s, acc, csize);
    }
#pragma unroll
    for (int i = 0; i < kQT; ++i) {
      const int uni = p.qcnt[qi[i] * kCntStride + k] + csize - acc[i];
      // strictly better than the kept shift, as fractions; a union of 0 is 0 / 1
      if (k == 0 || (long long)acc[i] * max(best_u[i], 1) > (long long)best_i[i] * max(uni, 1)) {
        best_i[i] = acc[i];
        best_u[i] = uni;
        best_k[i] = k;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < kQT; ++i) {
    s_inter[i][tid] = live ? best_i[i] : -1;
    s_union[i][tid] = live ? best_u[i] : 1;
    s_shift[i][tid] = rm_shift_of(best_k[i]);
    if (live && p.tab_inter && q0 + i < p.na) {
      const long long e = (long long)(q0 + i) * p.nb + b;
      p.tab_inter[e] = best_i[i];
      p.tab_union[e] = best_u[i];
      p.tab_shift[e] = rm_shift_of(best_k[i]);
    }
  }
  __syncthreads();
  // the chunk's top-k per query: one wave per query at a time, four candidates per lane
  const int lane = tid & 63, wave = tid >> 6;
  for (int i = wave; i < kQT && q0 + i < p.na; i += kChunk / 64) {
    RmCand prev = {0, 0, -1};
    int32_t* out = p.part + ((long long)(q0 + i) * p.nchunks + chunk) * p.topk * 4;
    for (int r = 0; r < p.topk; ++r) {
      RmCand mine = {-1, 1, kNoIdx};
#pragma unroll
      for (int j = 0; j < kChunk / 64; ++j) {
        const int e = lane + 64 * j;
        const RmCand c = {s_inter[i][e], s_union[i][e], e};
        if (c.inter >= 0 && (r == 0 || rm_before(prev, c)) && rm_before(c, mine)) mine = c;
      }
      const RmCand w = rm_wave_first(mine);
      if (lane == 0) {
        const bool any = w.inter >= 0;
        out[r * 4 + 0] = any ? chunk * kChunk + w.idx : -1;
        out[r * 4 + 1] = any ? s_shift[i][any ? w.idx : 0] : 0;
        out[r * 4 + 2] = any ? w.inter : 0;
        out[r * 4 + 3] = any ? w.uni : 0;
      }
      if (w.inter < 0) {                                                        // the chunk has no more candidates: the rest of the list is empty
        for (int e = (r + 1) * 4 + lane; e < p.topk * 4; e += 64) out[e] = (e & 3) == 0 ? -1 : 0;
        break;
      }
      prev = w;
    }
  }
}

// ------------------------------------------------------------------ merge: a wave per query over its partial lists, in chunk order
__global__ __launch_bounds__(64) void roll_match_merge_kernel(const int32_t* __restrict__ part, int nchunks, int topk,
                                                              int32_t* __restrict__ top_index, int32_t* __restrict__ top_shift,
                                                              int32_t* __restrict__ top_inter, int32_t* __restrict__ top_union) {
  const int q = blockIdx.x, lane = threadIdx.x;
  const int32_t* in = part + (long long)q * nchunks * topk * 4;
  const long long n = (long long)nchunks * topk;
  RmCand prev = {0, 0, -1};
  int shift_prev = 0;
  bool done = false;
  for (int r = 0; r < topk; ++r) {
    RmCand mine = {-1, 1, kNoIdx};
    int shift = 0;
    if (!done)
      for (long long e = lane; e < n; e += 64) {
        const RmCand c = {in[e * 4 + 2], in[e * 4 + 3], in[e * 4 + 0]};
        if (c.idx >= 0 && (r == 0 || rm_before(prev, c)) && rm_before(c, mine)) {
          mine = c;
          shift = in[e * 4 + 1];
        }
      }
    const RmCand w = rm_wave_first(mine);
    // the winner's shift lives in the lane that proposed it (indices are unique)
    const unsigned long long owner = __ballot(mine.idx == w.idx && w.inter >= 0);
    shift_prev = owner ? __shfl(shift, __builtin_ctzll(owner)) : 0;
    const bool any = w.inter >= 0;
    if (lane == 0) {
      top_index[q * topk + r] = any ? w.idx : -1;
      top_shift[q * topk + r] = any ? shift_prev : 0;
      top_inter[q * topk + r] = any ? w.inter : 0;
      top_union[q * topk + r] = any ? w.uni : 0;
    }
    done = !any;
    prev = w;
  }
}

size_t roll_match_workspace_bytes(int na, int nb, int topk) {
  if (na <= 0 || nb <= 0 || topk < 1 || topk > PF_ROLL_MATCH_MAX_TOPK) return 0;
  const size_t nchunks = ((size_t)nb + kChunk - 1) / kChunk;
  return 4 * ((size_t)na * kCntStride + (size_t)na * nchunks * topk * 4);
}

int launch_roll_match(const pf_roll_match_args& a, hipStream_t stream) {
  PF_REQUIRE(a.a_bits && a.a_starts && a.b_bits && a.b_starts, "roll_match: null input (a_bits %p, a_starts %p, b_bits %p, b_starts %p)",
             (const void*)a.a_bits, (const void*)a.a_starts, (const void*)a.b_bits, (const void*)a.b_starts);
  PF_REQUIRE(a.na > 0 && a.nb > 0 && a.steps > 0, "roll_match: bad shape (na = %d, nb = %d, steps = %d)", a.na, a.nb, a.steps);
  PF_REQUIRE(a.na <= kQT * 65535, "roll_match: na = %d is more than one call takes (%d)", a.na, kQT * 65535);
  PF_REQUIRE(a.shifts >= 0 && a.shifts <= PF_ROLL_MATCH_MAX_SHIFTS, "roll_match: shifts = %d outside 0..%d", a.shifts, PF_ROLL_MATCH_MAX_SHIFTS);
  PF_REQUIRE(a.topk >= 1 && a.topk <= PF_ROLL_MATCH_MAX_TOPK, "roll_match: topk = %d outside 1..%d", a.topk, PF_ROLL_MATCH_MAX_TOPK);
  PF_REQUIRE(a.reserved == 0, "roll_match: reserved = %d must be 0", a.reserved);
  PF_REQUIRE(a.top_index && a.top_shift && a.top_inter && a.top_union, "roll_match: null output (top_index %p, top_shift %p, top_inter %p, top_union %p)",
             (void*)a.top_index, (void*)a.top_shift, (void*)a.top_inter, (void*)a.top_union);
  const int ntab = (a.tab_inter != nullptr) + (a.tab_union != nullptr) + (a.tab_shift != nullptr);
  PF_REQUIRE(ntab == 0 || ntab == 3, "roll_match: the dense tables go together: give all three or none (tab_inter %p, tab_union %p, tab_shift %p)",
             (void*)a.tab_inter, (void*)a.tab_union, (void*)a.tab_shift);
  PF_REQUIRE(a.workspace, "roll_match: null workspace (pf_roll_match_workspace_bytes(na, nb, topk) bytes)");
  const size_t need = roll_match_workspace_bytes(a.na, a.nb, a.topk);
  PF_REQUIRE(a.workspace_bytes >= need, "roll_match: workspace of %zu bytes, %zu needed", (size_t)a.workspace_bytes, need);
  const uintptr_t a16 = (uintptr_t)a.a_bits | (uintptr_t)a.b_bits | (uintptr_t)a.workspace;
  const uintptr_t a4 = (uintptr_t)a.a_starts | (uintptr_t)a.b_starts | (uintptr_t)a.top_index | (uintptr_t)a.top_shift | (uintptr_t)a.top_inter |
                       (uintptr_t)a.top_union | (uintptr_t)a.tab_inter | (uintptr_t)a.tab_union | (uintptr_t)a.tab_shift;
  PF_REQUIRE(a16 % 16 == 0 && a4 % 4 == 0, "roll_match: a_bits, b_bits and workspace must be 16-byte aligned, every other pointer 4-byte");
  const int nshift = 2 * a.shifts + 1, nchunks = cdiv(a.nb, kChunk);
  int32_t* qcnt = static_cast<int32_t*>(a.workspace);
  int32_t* part = qcnt + (size_t)a.na * kCntStride;
  hipLaunchKernelGGL(roll_match_counts_kernel, dim3(a.na), dim3(64), 0, stream, static_cast<const uint32_t*>(a.a_bits), a.a_starts, a.steps, nshift,
                     qcnt);
  RmMatch p = {static_cast<const uint32_t*>(a.a_bits), a.a_starts, static_cast<const uint32_t*>(a.b_bits), a.b_starts, qcnt, part,
               a.tab_inter, a.tab_union, a.tab_shift, a.na, a.nb, a.steps, nshift, a.topk, nchunks};
  hipLaunchKernelGGL(roll_match_kernel, dim3(nchunks, cdiv(a.na, kQT)), dim3(kChunk), 0, stream, p);
  hipLaunchKernelGGL(roll_match_merge_kernel, dim3(a.na), dim3(64), 0, stream, part, nchunks, a.topk, a.top_index, a.top_shift, a.top_inter,
                     a.top_union);
  PF_CHECK_HIP(hipGetLastError());
  return PF_OK;
}

}  // namespace pf
