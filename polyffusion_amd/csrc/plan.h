// plan.h - host machinery shared by the model handles (pf_unet, pf_ddpm, pf_encoder, pf_decoder): the weight table that maps a
// reference state_dict key to its place in the ONE packed blob (every handle resolves its keys to blob offsets when it is created),
// and the plan context that carves the workspace and accounts for the launches of a forward.  Each handle writes its forward once, as
// a walk over a PlanCtx: a dry run of it sizes the workspace and counts the launches, a live run of it enqueues.
#pragma once
#include <map>
#include <string>
#include <vector>
#include "pf_internal.h"

namespace pf {

// (fp16 build only: bf16 pieces have fp32's range)
#define X3_RANGE_MSG "%s: a weight exceeds what this library's fp16 split packing holds (|w| <= 255.8; weights are stored times 2^8): load the checkpoint with the default library (bf16x3 / f32)"

// A GEMM weight region holds the fp32 packing [taps][K/4][Npad][4], then the split packing of the same byte count.
inline size_t gemm_floats(int taps, int K, int N) { return (size_t)taps * K * ((N + 63) / 64 * 64); }
inline size_t split_offset(int taps, int K, int N) { return gemm_floats(taps, K, N); }
// fp32 GEMM packing of [n_src][K](x taps) into columns n_off.. of an Npad-wide region
void pack_gemm(float* dst, const float* src, int n_src, int K, int taps, int Npad, int n_off);

// ---- weight table ----
enum DestKind {
  D_RAW,          // torch layout, copied
  D_GEMM,         // [N][K](x3x3) -> fp32 GEMM packing at column n_off of an Npad-wide region, + the split packing (K % 8 == 0)
  D_GEGLU_W,      // ff.net.0.proj weight: GEMM packing with the GeGLU column interleave, + its split packing
  D_GEGLU_B,      // ff.net.0.proj bias in the same column order
  D_CONVOUT,      // [Cout][Cin][3][3] -> [9][Cin][Cout] (head conv)
  D_UPFOLD,       // UpSample conv weight -> the split packing of its 4 parities x 4 taps
  D_WINO,         // 3x3 conv weight -> Winograd F(2x2, 3x3) split packing
  D_CONVT_F32,    // ConvTranspose2d(4, 2, 1) weight -> the fp32 packing of launch_convT_f32
  D_CONVT_BF3,    // the same weight folded into 16 taps -> the split GEMM packing (K % 8 == 0)
};
struct Dest { int kind; size_t off; int taps, K, N, Npad, n_off; };
// A key with no dests is accepted and dropped.  `optional`: it need not be supplied either (pack_missing does not count it).
struct Param { std::string key; std::vector<int64_t> shape; std::vector<Dest> dests; bool optional = false; bool packed = false; };

// blob offsets (in floats) of a linear layer / of one direction of a torch.nn.GRU layer
struct LinOff { size_t w, b; };
struct GruOff { size_t w_ih, w_hh, b_ih, b_hh; };

struct WeightTable {
  std::vector<Param> params;   // state_dict order
  std::map<std::string, int> index;
  size_t blob_floats = 0;
  const float* wdev = nullptr;   // the bound device blob

  size_t alloc(size_t nfloats) { const size_t o = blob_floats; blob_floats += (nfloats + 63) / 64 * 64; return o; }
  size_t alloc_gemm(int taps, int K, int N) { return alloc(2 * gemm_floats(taps, K, N)); }
  Param& add(const std::string& key, std::vector<int64_t> shape) {
    index[key] = (int)params.size();
    params.push_back(Param{key, std::move(shape)});
    return params.back();
  }
  // raw copy into a region of its own / into a pre-allocated region at a float offset
  size_t raw(const std::string& key, std::vector<int64_t> shape) {
    size_t n = 1;
    for (auto s : shape) n *= (size_t)s;
    const size_t off = alloc(n);
    raw_at(key, std::move(shape), off);
    return off;
  }
  void raw_at(const std::string& key, std::vector<int64_t> shape, size_t off) { add(key, std::move(shape)).dests.push_back(Dest{D_RAW, off, 1, 0, 0, 0, 0}); }
  // `name`.weight [N][K] and `name`.bias [N], raw
  LinOff linear(const std::string& name, int N, int K) {
    const size_t w = raw(name + ".weight", {N, K});
    return LinOff{w, raw(name + ".bias", {N})};
  }
  // the four raw tensors of each of the `ndir` directions of the one-layer GRU `name` (in -> hid), in state_dict order
  void gru(const std::string& name, int in, int hid, int ndir, GruOff* out) {
    for (int d = 0; d < ndir; ++d) {
      const std::string sfx = d ? "_l0_reverse" : "_l0";
      out[d].w_ih = raw(name + ".weight_ih" + sfx, {3 * hid, in});
      out[d].w_hh = raw(name + ".weight_hh" + sfx, {3 * hid, hid});
      out[d].b_ih = raw(name + ".bias_ih" + sfx, {3 * hid});
      out[d].b_hh = raw(name + ".bias_hh" + sfx, {3 * hid});
    }
  }
  // a GEMM weight [N][K] (taps == 1) or [N][K][3][3] (taps == 9) in a region of its own
  size_t gemm(const std::string& key, int N, int K, int taps) {
    const size_t off = alloc_gemm(taps, K, N);
    add(key, taps == 1 ? std::vector<int64_t>{N, K} : std::vector<int64_t>{N, K, 3, 3}).dests.push_back(Dest{D_GEMM, off, taps, K, N, (N + 63) / 64 * 64, 0});
    return off;
  }

  // the bodies of the <model>_param_info / _pack_param / _pack_missing / _bind_weights entry points (`fn`: the entry point's name,
  // `model`: what the table belongs to, for the messages)
  int param_info(const char* fn, int i, char* key_buf, size_t key_buf_len, int64_t shape[4], int* ndim) const;
  int pack_param(const char* fn, const char* model, const char* key, const float* src, const int64_t* shape, int ndim, void* host_blob);
  int pack_missing(char* buf, size_t buf_len) const;
  int bind(const char* fn, const void* dev_blob, bool aligned);
};

// ---- plan context ----
struct ProfRec { int kind; double flops, direct; };   // direct: operations of the layer's direct form (differs for Winograd launches)
// hipEvents around every launch of a profiled forward, owned by the model handle and attached to the live context of that forward
struct Profiler {
  std::vector<hipEvent_t> ev;   // two per record
  std::vector<ProfRec> rec;
  ~Profiler() { for (auto e : ev) (void)hipEventDestroy(e); }
  void begin(const ProfRec& r, hipStream_t s) {
    while (ev.size() < 2 * (rec.size() + 1)) { hipEvent_t e; (void)hipEventCreate(&e); ev.push_back(e); }
    rec.push_back(r);
    (void)hipEventRecord(ev[2 * rec.size() - 2], s);
  }
  void end(hipStream_t s) { (void)hipEventRecord(ev[2 * rec.size() - 1], s); }
};

struct PlanSize {
  size_t persist, temp;   // workspace: persistent region, then the temporaries
  int n_launch;
  double flops;
  size_t bytes() const { return persist + temp; }
};

// The workspace arena of a plan (two bump allocators: persistent tensors, per-layer temporaries recycled by treset) and its launch
// accounting.  A dry run carries no pointers and enqueues nothing; it only records the high-water marks, launches and operations.
struct PlanCtx {
  hipStream_t s = nullptr;
  bool dry = true;
  char* base = nullptr;
  size_t persist_off = 0, temp_base = 0, temp_off = 0, persist_max = 0, temp_max = 0;
  const float* W = nullptr;   // the bound weight blob
  int B = 0;
  int rc = PF_OK;
  int n_launch = 0;
  double flops = 0.0;
  Profiler* prof = nullptr;

  float* palloc(size_t nfloats) {
    const size_t o = persist_off;
    persist_off += align_up(nfloats * 4, 256);
    if (persist_off > persist_max) persist_max = persist_off;
    return dry ? nullptr : (float*)(base + o);
  }
  float* talloc(size_t nfloats) {
    const size_t o = temp_off;
    temp_off += align_up(nfloats * 4, 256);
    if (temp_off > temp_max) temp_max = temp_off;
    return dry ? nullptr : (float*)(base + temp_base + o);
  }
  void treset() { temp_off = 0; }
  const float* w(size_t off) const { return dry ? nullptr : W + off; }
  // the split packing of the GEMM region at `off` (dry: a non-null placeholder, it only says that the operand exists)
  const void* w_split(size_t off, int taps, int K, int N) const { return dry ? (const void*)16 : (const void*)(W + off + split_offset(taps, K, N)); }

  // One launch (or `count` launches enqueued together) of `flops` operations: counted on every run, one profile record when a
  // profiler is attached, and `enqueue()` (returns a PF_* code) called only on a live run whose earlier launches all succeeded.
  template <class F>
  void launch(int kind, double fl, F&& enqueue, int count = 1, double direct = -1.0) {
    n_launch += count;
    flops += fl;
    if (dry) return;
    if (prof) prof->begin(ProfRec{kind, fl, direct < 0.0 ? fl : direct}, s);
    if (rc == PF_OK) rc = enqueue();
    if (prof) prof->end(s);
  }

  // live run in `ws` (aligned to `align` bytes, a power of two), on `stream`, with the bound blob: checks the workspace against the
  // plan's dry-run sizes, then carves it
  int use_workspace(const char* fn, void* ws, size_t ws_bytes, const PlanSize& z, void* stream, const float* wdev, size_t align = 256) {
    PF_REQUIRE(((uintptr_t)ws & (align - 1)) == 0, "%s: workspace must be %zu-byte aligned", fn, align);
    if (ws_bytes < z.bytes()) return set_error(PF_EINVAL, "%s: workspace too small (%zu < %zu)", fn, ws_bytes, z.bytes());
    dry = false;
    base = (char*)ws;
    temp_base = z.persist;
    s = (hipStream_t)stream; W = wdev;
    return PF_OK;
  }
};

// sizes of the plan `run(ctx)` walks, from a dry run of a copy of `c`
template <class Ctx, class Run>
PlanSize plan_sizes(Ctx c, Run&& run) {
  c.dry = true;
  c.prof = nullptr;
  run(c);
  return PlanSize{align_up(c.persist_max, 4096), align_up(c.temp_max, 4096), c.n_launch, c.flops};
}

inline pf_conv_args conv_base(const float* x0, int c0, const float* x1, int c1, int B, int hin, int win, int ks, const float* wgt, int n,
                              float* out) {
  pf_conv_args a;
  memset(&a, 0, sizeof a);
  a.x0 = x0; a.c0 = c0; a.x1 = x1; a.c1 = c1; a.batch = B; a.hin = hin; a.win = win; a.ks = ks; a.stride = 1;
  a.w = wgt; a.n = n; a.out = out; a.ld_out = n;
  return a;
}

}  // namespace pf
