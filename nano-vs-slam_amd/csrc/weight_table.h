// The weight table behind kp2d_weight_info / kp2d_set_weight and their kp2d_lg_* twins: the state-dict tensors a handle
// consumes (key and shape, in the reference's registration order) and the host copies received so far.  No HIP.  What the two
// ABIs do differently — which arguments may be null, their refusal's message, the ignored BatchNorm counter — stays at their
// call sites (kp2d_api.cpp, lightglue_api.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "api_common.h"

namespace kp2d {

struct WeightSpec {
  std::string key;
  std::vector<int64_t> shape;
  size_t numel() const {
    size_t n = 1;
    for (auto s : shape) n *= (size_t)s;
    return n;
  }
};

// row `index` (in range: the caller's check) into those of key / shape / ndim that are not null; pad_shape: the entries of
// shape[4] past ndim become 1 instead of staying untouched
inline void weight_info(const std::vector<WeightSpec>& specs, int index, const char** key, int64_t shape[4], int* ndim, bool pad_shape) {
  const WeightSpec& s = specs[index];
  if (key) *key = s.key.c_str();
  if (ndim) *ndim = (int)s.shape.size();
  if (shape)
    for (size_t i = 0; i < 4; ++i) {
      if (i < s.shape.size()) shape[i] = s.shape[i];
      else if (pad_shape) shape[i] = 1;
    }
}

// one tensor of the state dict into `host`; a key the table lacks or another shape is KP2D_ERR_WEIGHT
inline int set_weight(const std::vector<WeightSpec>& specs, const std::map<std::string, int>& index,
                      std::map<std::string, std::vector<float>>& host, const char* key, const float* data, const int64_t* shape, int ndim) {
  auto it = index.find(key);
  if (it == index.end()) return fail(KP2D_ERR_WEIGHT, "unexpected key '%s'", key);
  const WeightSpec& s = specs[it->second];
  bool same = (int)s.shape.size() == ndim;
  for (int i = 0; same && i < ndim; ++i) same = s.shape[i] == shape[i];
  if (!same) return fail(KP2D_ERR_WEIGHT, "shape mismatch for '%s'", key);
  host[key].assign(data, data + s.numel());
  return KP2D_OK;
}

}  // namespace kp2d
