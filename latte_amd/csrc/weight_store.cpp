#include "weight_store.h"

namespace latte {

DeviceArena::~DeviceArena() {
  for (void* p : blocks_) (void)hipFree(p);
}

void DeviceArena::release(void* p) {
  blocks_.erase(std::remove(blocks_.begin(), blocks_.end(), p), blocks_.end());
  (void)hipFree(p);
}

WeightSlot& WeightSlots::add(const std::string& key, int64_t numel, int kind, void* dst, int rows, int cols) {
  WeightSlot s;
  s.key = key; s.numel = numel; s.kind = kind; s.dst = dst; s.rows = rows; s.cols = cols;
  index_[key] = size();
  slots_.push_back(s);
  stage_numel_ = std::max(stage_numel_, numel);
  return slots_.back();
}

int WeightSlots::find(const char* who, const char* key, WeightSlot** out) {
  auto it = index_.find(key);
  if (it == index_.end()) return fail(LATTE_ERR_INVALID, std::string(who) + ": unexpected key '" + key + "'");
  *out = &slots_[it->second];
  return LATTE_OK;
}

int WeightSlots::begin_load(const char* who, const char* key, const float* data, int64_t numel, bool on_device, hipStream_t st,
                            WeightSlot** out, const float** src) {
  if (int rc = find(who, key, out)) return rc;
  WeightSlot& s = **out;
  if (s.optional) { s.loaded = true; return LATTE_OK; }
  if (numel != s.numel)
    return fail(LATTE_ERR_INVALID, std::string(who) + ": size mismatch for '" + key + "': got " + std::to_string(numel) + ", expected " +
                                       std::to_string(s.numel));
  *src = data;
  if (!on_device) {
    LATTE_HIP(hipMemcpyAsync(stage_, data, sizeof(float) * numel, hipMemcpyHostToDevice, st));
    *src = stage_;
  }
  return LATTE_OK;
}

int WeightSlots::end_load(WeightSlot& s, bool on_device, hipStream_t st) {
  if (!on_device) LATTE_HIP(hipStreamSynchronize(st));
  s.loaded = true;
  return LATTE_OK;
}

int WeightSlots::check_loaded() const {
  for (const auto& s : slots_) {
    bool ok = s.loaded || s.optional;
    if (!ok && s.group >= 0)
      for (const auto& o : slots_) ok = ok || (o.group == s.group && o.loaded);
    if (!ok) return fail(LATTE_ERR_STATE, "Missing key(s) in state_dict: \"" + s.key + "\"");
  }
  return LATTE_OK;
}

}  // namespace latte
