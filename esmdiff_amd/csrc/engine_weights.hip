// engine_weights.hip — the weight loader of libesmdiff_hip.so: every create (engine, decoder, encoder) reads its table through
// Table / need and fills its buffers through load_f32 / load_linear (declared in engine.h).  The loader asks of its owner only
// an eng::Owner: the error string and the list of allocations that destroy frees.
#include "engine.h"

using namespace ed;

namespace eng {

Table::Table(const esmdiff_weight* table, int n, const char* prefix) : prefix(prefix) {
  for (int i = 0; i < n; ++i)
    if (table[i].name) m[table[i].name] = &table[i];
}

const esmdiff_weight* Table::find(const std::string& name) const {
  auto it = m.find(name);
  if (it == m.end() && !prefix.empty()) it = m.find(prefix + name);
  return it == m.end() ? nullptr : it->second;
}

int64_t numel(const esmdiff_weight* w) {
  int64_t n = 1;
  for (int i = 0; i < w->ndim; ++i) n *= w->shape[i];
  return n;
}

int need(Owner* o, const Table& t, const std::string& name, std::initializer_list<int64_t> shape, const esmdiff_weight** out) {
  const esmdiff_weight* w = t.find(name);
  if (!w) return fail(o, ESMDIFF_E_MISSING, "missing weight '%s' (state dict is loaded strictly, checkpoint_utils.py:64)", name.c_str());
  if (w->ndim != (int)shape.size()) return fail(o, ESMDIFF_E_SHAPE, "weight '%s': ndim %d, expected %zu", name.c_str(), w->ndim, shape.size());
  int i = 0;
  for (int64_t s : shape) {
    if (w->shape[i] != s) return fail(o, ESMDIFF_E_SHAPE, "weight '%s': dim %d is %lld, expected %lld", name.c_str(), i, (long long)w->shape[i], (long long)s);
    ++i;
  }
  if (w->dtype != ESMDIFF_F32 && w->dtype != ESMDIFF_BF16) return fail(o, ESMDIFF_E_SHAPE, "weight '%s': unsupported dtype %d", name.c_str(), w->dtype);
  if (!w->data) return fail(o, ESMDIFF_E_INVALID, "weight '%s': null data", name.c_str());
  *out = w;
  return 0;
}

int load_f32(Owner* o, const Table& t, const std::string& name, std::initializer_list<int64_t> shape, float** dst, int64_t pad_to) {
  const esmdiff_weight* w;
  if (int r = need(o, t, name, shape, &w)) return r;
  const int64_t n = numel(w), n_p = pad_to > n ? pad_to : n;
  if (int r = dalloc(o, dst, (size_t)n_p, n_p != n)) return r;
  HIP_TRY(o, launch_to_f32(w->data, w->dtype, *dst, n, 0));
  return 0;
}

int load_linear(Owner* o, const Table& t, const std::string& name, std::initializer_list<int64_t> shape, Linear::Form form,
                Linear* dst, int64_t pad_rows, int swiglu_h, bool f16, uint32_t* scratch_bits) {
  const esmdiff_weight* w;
  if (int r = need(o, t, name, shape, &w)) return r;
  const int64_t n = numel(w), rows = w->shape[0], K = n / rows;
  const int64_t rows_p = form != Linear::F32 && pad_rows > rows ? pad_rows : rows;
  if (form == Linear::SPLIT) {
    if (K % 128 || rows_p % 256) return fail(o, ESMDIFF_E_SHAPE, "weight '%s': [%lld, %lld] does not fit the split GEMM (rows %% 256, K %% 128)", name.c_str(), (long long)rows_p, (long long)K);
    uint16_t* p;
    if (int r = dalloc(o, &p, (size_t)(rows_p * 3 * K), rows_p != rows)) return r;
    dst->w = p;
    HIP_TRY(o, split_weight(w->data, w->dtype, p, rows, (int)K, scratch_bits, &dst->inv, swiglu_h));
  } else if (form == Linear::F32) {
    float* p;
    if (int r = dalloc(o, &p, (size_t)n)) return r;
    dst->w = p;
    HIP_TRY(o, launch_to_f32(w->data, w->dtype, p, n, 0));
  } else {
    bf16_t* p;
    if (int r = dalloc(o, &p, (size_t)(rows_p * K), rows_p != rows)) return r;
    dst->w = p;
    if (swiglu_h) {
      if (ED_KN(f16, launch_interleave_swiglu(w->data, w->dtype, p, swiglu_h, (int)K, 0)) != hipSuccess)
        return fail(o, ESMDIFF_E_HIP, "interleave_swiglu launch failed");
    } else {
      HIP_TRY(o, ED_KN(f16, launch_to_bf16(w->data, w->dtype, p, n, 0)));
    }
  }
  dst->form = form;
  return 0;
}

}  // namespace eng
