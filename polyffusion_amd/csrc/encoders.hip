// encoders.hip - frozen condition encoders (run once per generation, before the step loop).
//   chord:   RnnEncoder(36 -> bi-GRU 512 -> mu 512)                (dl_modules/chord_enc.py:5-22)
//   texture: TextureEncoder(conv 4x12 -> ReLU -> pool -> fc1 -> fc2 -> bi-GRU 1024 -> mu 256)
//                                                                   (dl_modules/txt_enc.py:5-35)
// Only Normal(mu, .).mean is consumed downstream (models/model_sdf.py:99,157), so linear_var is
// accepted at pack time (checkpoint compatibility) and ignored - unless the encoder was created
// with_scale (pf_encoder_create_dist): Polydis samples from the Normal (polydis/model.py:188-239), so
// linear_var.* then has a place at the end of the blob and pf_encoder_forward_dist also writes
// scale = exp(linear_var(h)) (polydis/ptvae.py:25-27, :115-117).  Weights keep their torch
// row-major layout; every contraction is the batched mat-vec kernel (weights stream once per
// 8 samples), the recurrence is one mat-vec + one gate kernel per time step.
#include <memory>
#include <string>
#include <vector>
#include "plan.h"

using namespace pf;

struct pf_encoder {
  int kind, input_dim, emb, hidden, z, nch;
  bool with_scale = false;
  WeightTable wt;
  // blob offsets of everything the forward reads, resolved at create
  LinOff note_emb{}, cnn{}, fc1{}, fc2{}, mu{}, var{};
  GruOff notes_gru[2] = {}, gru[2] = {};   // pnotree: the GRU over the notes of a step; the GRU over time (pnotree: the 32 steps)
  void add_unused(const std::string& key, std::vector<int64_t> shape) { wt.add(key, std::move(shape)).optional = true; }
};

extern "C" {

int pf_encoder_create_dist(int kind, int input_dim, int emb_size, int hidden_dim, int z_dim, int num_channel, int with_scale,
                           pf_encoder** out) {
  PF_REQUIRE(out && (kind == PF_ENC_CHORD || kind == PF_ENC_TEXTURE || kind == PF_ENC_PNOTREE), "pf_encoder_create: bad kind");
  PF_REQUIRE(hidden_dim > 0 && z_dim > 0, "pf_encoder_create: bad dims");
  // linear_mu contracts over 2 * hidden_dim, and the batched mat-vec takes K <= 2048: refused here, not after the GRU has been enqueued
  PF_REQUIRE(hidden_dim <= 1024, "pf_encoder_create: hidden_dim=%d above 1024 (linear_mu's mat-vec takes K = 2 * hidden_dim <= 2048)", hidden_dim);
  PF_REQUIRE(!with_scale || kind != PF_ENC_PNOTREE, "pf_encoder_create_dist: the scale head exists for the chord and texture encoders only");
  std::unique_ptr<pf_encoder> e(new pf_encoder());
  e->with_scale = with_scale != 0;
  e->kind = kind; e->input_dim = input_dim; e->emb = emb_size; e->hidden = hidden_dim; e->z = z_dim; e->nch = num_channel;
  WeightTable& wt = e->wt;
  int gru_in = input_dim;
  const char* unused = "linear_var";   // accepted and ignored
  if (kind == PF_ENC_PNOTREE) {   // dl_modules/pianotree_enc.py:43-59
    PF_REQUIRE(input_dim > 5 && emb_size > 0 && num_channel > 0, "pf_encoder_create: pianotree encoder needs input_dim, emb_size and the note-GRU size");
    e->note_emb = wt.linear("note_embedding", emb_size, input_dim);
    wt.gru("enc_notes_gru", emb_size, num_channel, 2, e->notes_gru);
    gru_in = 2 * num_channel;
    unused = "linear_std";
  } else if (kind == PF_ENC_TEXTURE) {
    PF_REQUIRE(num_channel > 0 && emb_size > 0, "pf_encoder_create: texture encoder needs num_channel and emb_size");
    e->cnn.w = wt.raw("cnn.0.weight", {num_channel, 1, 4, 12});
    e->cnn.b = wt.raw("cnn.0.bias", {num_channel});
    e->fc1 = wt.linear("fc1", 1000, num_channel * 29);
    e->fc2 = wt.linear("fc2", emb_size, 1000);
    gru_in = emb_size;
  }
  PF_REQUIRE(gru_in > 0 && gru_in <= 2048 && emb_size <= 2048 && (kind != PF_ENC_TEXTURE || num_channel * 29 <= 2048),
             "pf_encoder_create: a contraction longer than the mat-vec's 2048 (GRU input %d, emb_size %d, num_channel %d)", gru_in, emb_size, num_channel);
  wt.gru(kind == PF_ENC_PNOTREE ? "enc_time_gru" : "gru", gru_in, hidden_dim, 2, e->gru);
  e->mu = wt.linear("linear_mu", z_dim, 2 * hidden_dim);
  if (e->with_scale) {   // last in the table: everything before it sits where it does without the scale head
    e->var = wt.linear("linear_var", z_dim, 2 * hidden_dim);
  } else {
    e->add_unused(std::string(unused) + ".weight", {z_dim, 2 * hidden_dim});
    e->add_unused(std::string(unused) + ".bias", {z_dim});
  }
  *out = e.release();
  return PF_OK;
}
int pf_encoder_create(int kind, int input_dim, int emb_size, int hidden_dim, int z_dim, int num_channel, pf_encoder** out) {
  return pf_encoder_create_dist(kind, input_dim, emb_size, hidden_dim, z_dim, num_channel, 0, out);
}

void pf_encoder_destroy(pf_encoder* e) { delete e; }
size_t pf_encoder_weight_bytes(const pf_encoder* e) { return e ? e->wt.blob_floats * sizeof(float) : 0; }

int pf_encoder_pack_param(pf_encoder* e, const char* key, const float* src, const int64_t* shape, int ndim, void* host_blob) {
  PF_REQUIRE(e, "pf_encoder_pack_param: null argument");
  return e->wt.pack_param("pf_encoder_pack_param", "encoder", key, src, shape, ndim, host_blob);
}
int pf_encoder_pack_missing(const pf_encoder* e, char* buf, size_t buf_len) { return e ? e->wt.pack_missing(buf, buf_len) : set_error(PF_EINVAL, "null handle"); }
// (no alignment requirement, unlike the UNets: an encoder blob may be a slice of a larger buffer)
int pf_encoder_bind_weights(pf_encoder* e, const void* dev_blob) {
  PF_REQUIRE(e, "pf_encoder_bind_weights: null argument");
  return e->wt.bind("pf_encoder_bind_weights", dev_blob, false);
}

}  // extern "C"

namespace {

// One bidirectional GRU layer over x [R * T][in] (row r, step t at r * T + t): per direction the input projection of every step, then
// T x (W_hh mat-vec + gate launch).  Returns [R][2H] = [h_forward | h_backward] at the end of each direction.  `masked`: rows end at
// their own length lens[r] (the masked gate kernel, which finds step t of its direction itself).
const float* bigru(PlanCtx& c, const GruOff (&g)[2], const float* x, int in, int R, int T, int H, bool masked, const int* lens) {
  const size_t gi_floats = (size_t)R * T * 3 * H;
  float* gi0 = c.palloc(gi_floats);
  float* gi1 = masked ? gi0 : c.palloc(gi_floats);   // the masked (note) GRU's two projections take turns in one buffer
  float* gh = c.palloc((size_t)R * 3 * H);
  float* hcat = c.palloc((size_t)R * 2 * H);
  c.launch(PF_K_SMALL, 0.0, [&] { PF_CHECK_HIP(hipMemsetAsync(hcat, 0, (size_t)R * 2 * H * sizeof(float), c.s)); return PF_OK; }, 0);
  for (int d = 0; d < 2; ++d) {
    float* gi = d ? gi1 : gi0;
    c.launch(PF_K_SMALL, 0.0, [&] { return launch_matvec(x, in, c.w(g[d].w_ih), c.w(g[d].b_ih), gi, 3 * H, R * T, 3 * H, in, c.s); });
    for (int step = 0; step < T; ++step) {
      c.launch(PF_K_SMALL, 0.0, [&] { return launch_matvec(hcat + d * H, 2 * H, c.w(g[d].w_hh), c.w(g[d].b_hh), gh, 3 * H, R, 3 * H, H, c.s); });
      c.launch(PF_K_SMALL, 0.0, [&] {
        float* h = hcat + d * H;   // row stride 2H
        if (masked) return launch_gru_gates_masked(gi, gh, h, 2 * H, R, H, T, lens, step, d, c.s);
        return launch_gru_gates(gi + (size_t)(d ? T - 1 - step : step) * 3 * H, T * 3 * H, gh, h, 2 * H, R, H, c.s);
      });
    }
  }
  return hcat;
}

// The forward of every encoder kind, dry or live.  n_step: T of the chord encoder, max_simu_note of the PianoTree encoder (the texture
// encoder always has 8 steps).  c.B = batch.
int enc_run(const pf_encoder* e, PlanCtx& c, const float* x, int n_step, float* mu, float* scale) {
  const int B = c.B, H = e->hidden;
  const float* h;
  if (e->kind == PF_ENC_PNOTREE) {
    // PianoTreeEncoder.forward (dl_modules/pianotree_enc.py:97-121): embed every grid row, run the bidirectional note GRU over the
    // (variable number of) notes of each of the B*32 time steps, then the bidirectional time GRU over the 32 steps, then linear_mu
    const int S = n_step, E = e->emb, Hn = e->nch, N = B * 32, P = e->input_dim - 5;
    float* emb = c.palloc((size_t)N * S * E);
    int* lens = reinterpret_cast<int*>(c.palloc(N));
    c.launch(PF_K_SMALL, 0.0, [&] { return launch_pnotree_embed(x, c.w(e->note_emb.w), c.w(e->note_emb.b), emb, N * S, E, P, c.s); });
    c.launch(PF_K_SMALL, 0.0, [&] { return launch_pnotree_lengths(x, lens, N, S, P, c.s); });
    const float* hn = bigru(c, e->notes_gru, emb, E, N, S, Hn, true, lens);
    h = bigru(c, e->gru, hn, 2 * Hn, B, 32, H, false, nullptr);
  } else if (e->kind == PF_ENC_TEXTURE) {
    const int K1 = e->nch * 29;  // rows of the un-permuted [B,8,-1] view (txt_enc.py:27)
    float* feat = c.palloc((size_t)B * 8 * K1);
    float* a1 = c.palloc((size_t)B * 8 * 1000);
    float* em = c.palloc((size_t)B * 8 * e->emb);
    c.launch(PF_K_SMALL, 0.0, [&] { return launch_txt_frontend(x, c.w(e->cnn.w), c.w(e->cnn.b), feat, B, e->nch, c.s); });
    c.launch(PF_K_SMALL, 0.0, [&] { return launch_matvec(feat, K1, c.w(e->fc1.w), c.w(e->fc1.b), a1, 1000, B * 8, 1000, K1, c.s); });
    c.launch(PF_K_SMALL, 0.0, [&] { return launch_matvec(a1, 1000, c.w(e->fc2.w), c.w(e->fc2.b), em, e->emb, B * 8, e->emb, 1000, c.s); });
    h = bigru(c, e->gru, em, e->emb, B, 8, H, false, nullptr);
  } else {
    h = bigru(c, e->gru, x, e->input_dim, B, n_step, H, false, nullptr);   // x [B][T][input_dim]
  }
  c.launch(PF_K_SMALL, 0.0, [&] { return launch_matvec(h, 2 * H, c.w(e->mu.w), c.w(e->mu.b), mu, e->z, B, e->z, 2 * H, c.s); });
  if (scale) c.launch(PF_K_SMALL, 0.0, [&] { return launch_matvec_exp(h, 2 * H, c.w(e->var.w), c.w(e->var.b), scale, e->z, B, e->z, 2 * H, c.s); });
  return c.rc;
}

// The workspace is sized by batch alone, for the longest sequence a forward accepts (64 chord steps, 32 simultaneous notes): the walk
// of a shorter one carves the same buffers, each no larger, in the same order.
PlanSize enc_plan(const pf_encoder* e, int batch) {
  PlanCtx c;
  c.B = batch;
  return plan_sizes(c, [e](PlanCtx& d) { enc_run(e, d, nullptr, e->kind == PF_ENC_PNOTREE ? 32 : 64, nullptr, nullptr); });
}

int enc_forward(pf_encoder* e, const float* x, int batch, int n_step, float* mu, float* scale, void* workspace, size_t workspace_bytes,
                void* stream) {
  PF_REQUIRE(e && x && mu && workspace && batch > 0, "pf_encoder_forward: bad arguments");
  if (!e->wt.wdev) return set_error(PF_ESTATE, "pf_encoder_forward: weights not bound");
  PF_REQUIRE(e->kind == PF_ENC_TEXTURE || (n_step > 0 && n_step <= 64), "pf_encoder_forward: n_step must be in 1..64");
  PF_REQUIRE(e->kind != PF_ENC_PNOTREE || n_step <= 32, "pf_encoder_forward: at most 32 simultaneous notes");
  PlanCtx c;
  c.B = batch;
  const int rc = c.use_workspace("pf_encoder_forward", workspace, workspace_bytes, enc_plan(e, batch), stream, e->wt.wdev, 1);
  if (rc != PF_OK) return rc;
  return enc_run(e, c, x, n_step, mu, scale);
}

}  // namespace

extern "C" {

size_t pf_encoder_workspace_bytes(const pf_encoder* e, int batch) { return (e && batch > 0) ? enc_plan(e, batch).bytes() : 0; }

int pf_encoder_forward(pf_encoder* e, const float* x, int batch, int n_step, float* mu, void* workspace, size_t workspace_bytes,
                       void* stream) {
  return enc_forward(e, x, batch, n_step, mu, nullptr, workspace, workspace_bytes, stream);
}

int pf_encoder_forward_dist(pf_encoder* e, const float* x, int batch, int n_step, float* mu, float* scale, void* workspace,
                            size_t workspace_bytes, void* stream) {
  PF_REQUIRE(e && scale, "pf_encoder_forward_dist: bad arguments");
  PF_REQUIRE(e->kind != PF_ENC_PNOTREE, "pf_encoder_forward_dist: the PianoTree encoder has no scale head on this path (chord and texture encoders only)");
  PF_REQUIRE(e->with_scale, "pf_encoder_forward_dist: this encoder was created without the scale head (use pf_encoder_create_dist with with_scale = 1)");
  return enc_forward(e, x, batch, n_step, mu, scale, workspace, workspace_bytes, stream);
}

}  // extern "C"
