// plan.hip - the weight table's packing and the bodies of the per-model weight entry points (plan.h).
#include "plan.h"

namespace pf {

void pack_gemm(float* dst, const float* src, int n_src, int K, int taps, int Npad, int n_off) {
  for (int n = 0; n < n_src; ++n)
    for (int k = 0; k < K; ++k)
      for (int t = 0; t < taps; ++t)
        dst[(((size_t)t * (K / 4) + k / 4) * Npad + n_off + n) * 4 + (k & 3)] = src[((size_t)n * K + k) * taps + t];
}

namespace {

inline int geglu_col(int n, int inner) {  // torch row n of ff.net.0.proj -> packed column
  const int j = n < inner ? n : n - inner;
  return 64 * (j / 32) + (n < inner ? 0 : 32) + (j % 32);
}

// false when a weight does not fit the split's element type (fp16 build)
bool pack_one(const Param& ps, const float* src, float* blob) {
  size_t numel = 1;
  for (auto s : ps.shape) numel *= (size_t)s;
  bool fits = true;
  for (const Dest& d : ps.dests) {
    float* dst = blob + d.off;
    switch (d.kind) {
      case D_RAW: memcpy(dst, src, numel * sizeof(float)); break;
      case D_GEMM:
        pack_gemm(dst, src, d.N, d.K, d.taps, d.Npad, d.n_off);
        if (d.K % 8 == 0) fits = pack_gemm_bf3(dst + split_offset(d.taps, d.K, d.Npad), src, d.N, d.K, d.taps, d.Npad, d.n_off, nullptr) && fits;
        break;
      case D_UPFOLD: fits = pack_upfold_bf3(dst, src, d.N, d.K, d.Npad) && fits; break;
      case D_WINO: fits = pack_wino_bf3(dst, src, d.N, d.K) && fits; break;
      case D_GEGLU_W: {
        const int inner = d.N / 2;
        for (int n = 0; n < d.N; ++n)
          for (int k = 0; k < d.K; ++k) dst[((size_t)(k / 4) * d.Npad + geglu_col(n, inner)) * 4 + (k & 3)] = src[(size_t)n * d.K + k];
        std::vector<int> cm(d.N);
        for (int n = 0; n < d.N; ++n) cm[n] = geglu_col(n, inner);
        fits = pack_gemm_bf3(dst + split_offset(1, d.K, d.Npad), src, d.N, d.K, 1, d.Npad, 0, cm.data()) && fits;
        break;
      }
      case D_GEGLU_B: {
        const int inner = d.N / 2;
        for (int n = 0; n < d.N; ++n) dst[geglu_col(n, inner)] = src[n];
        break;
      }
      case D_CONVOUT:
        for (int co = 0; co < d.N; ++co)
          for (int ci = 0; ci < d.K; ++ci)
            for (int t = 0; t < 9; ++t) dst[((size_t)t * d.K + ci) * d.N + co] = src[((size_t)co * d.K + ci) * 9 + t];
        break;
      case D_CONVT_F32: pack_convT_f32(src, d.K, d.N, dst); break;
      case D_CONVT_BF3:
        if (d.K % 8 == 0) {
          std::vector<float> fold((size_t)16 * d.K * d.N);
          convT_fold(src, d.K, d.N, fold.data());
          fits = pack_gemm_bf3(dst, fold.data(), d.N, d.K, 16, d.Npad, 0, nullptr) && fits;
        }
        break;
    }
  }
  return fits;
}

}  // namespace

int WeightTable::param_info(const char* fn, int i, char* key_buf, size_t key_buf_len, int64_t shape[4], int* ndim) const {
  PF_REQUIRE(i >= 0 && i < (int)params.size() && key_buf && shape && ndim, "%s: bad arguments", fn);
  const Param& ps = params[i];
  snprintf(key_buf, key_buf_len, "%s", ps.key.c_str());
  *ndim = (int)ps.shape.size();
  for (int d = 0; d < 4; ++d) shape[d] = d < *ndim ? ps.shape[d] : 1;
  return PF_OK;
}

int WeightTable::pack_param(const char* fn, const char* model, const char* key, const float* src, const int64_t* shape, int ndim, void* host_blob) {
  PF_REQUIRE(key && src && shape && host_blob, "%s: null argument", fn);
  auto it = index.find(key);
  if (it == index.end()) return set_error(PF_ENOTFOUND, "unexpected key '%s' (not a parameter of this %s)", key, model);
  Param& ps = params[it->second];
  bool ok = ndim == (int)ps.shape.size();
  for (int d = 0; ok && d < ndim; ++d) ok = shape[d] == ps.shape[d];
  if (!ok) {
    std::string want, got;
    for (auto s : ps.shape) want += std::to_string(s) + ",";
    for (int d = 0; d < ndim; ++d) got += std::to_string(shape[d]) + ",";
    return set_error(PF_EINVAL, "size mismatch for '%s': expected [%s] got [%s]", key, want.c_str(), got.c_str());
  }
  if (!pack_one(ps, src, (float*)host_blob)) return set_error(PF_EINVAL, X3_RANGE_MSG, key);
  ps.packed = true;
  return PF_OK;
}

int WeightTable::pack_missing(char* buf, size_t buf_len) const {
  int n = 0;
  for (const Param& ps : params)
    if (!ps.packed && !ps.optional) {
      if (n == 0 && buf && buf_len) snprintf(buf, buf_len, "%s", ps.key.c_str());
      ++n;
    }
  return n;
}

int WeightTable::bind(const char* fn, const void* dev_blob, bool aligned) {
  PF_REQUIRE(dev_blob, "%s: null argument", fn);
  PF_REQUIRE(!aligned || ((uintptr_t)dev_blob & 255) == 0, "%s: blob must be 256-byte aligned", fn);
  wdev = (const float*)dev_blob;
  return PF_OK;
}

}  // namespace pf
