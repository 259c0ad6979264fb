// Host plumbing every engine shares (engine.cpp, t2v_engine.cpp, vae_engine.cpp, t5_engine.cpp; train_engine.cpp: the arena only):
// the device allocations an engine owns, and its table of weight slots under their state-dict keys with the frame of a load call
// around the engine's own `switch (kind)`.
#pragma once
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "common.h"

namespace latte {

// Every device block of one engine; freed with it (so `delete engine` is the whole error path of a create function).
class DeviceArena {
 public:
  DeviceArena() = default;
  DeviceArena(const DeviceArena&) = delete;
  DeviceArena& operator=(const DeviceArena&) = delete;
  ~DeviceArena();
  template <class T>
  int alloc(T** p, size_t count, bool zero = true) {   // an empty request still gets a valid 16-byte block
    const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
    void* q = nullptr;
    LATTE_HIP(hipMalloc(&q, bytes));
    blocks_.push_back(q);
    if (zero) LATTE_HIP(hipMemset(q, 0, bytes));
    *p = (T*)q;
    return LATTE_OK;
  }
  void release(void* p);   // frees one block early (hipFree synchronises the device: setup paths only)

 private:
  std::vector<void*> blocks_;
};

struct WeightSlot {
  std::string key;
  int64_t numel = 0;
  std::vector<int64_t> shape;   // T5 only: the expected shape (numel is its product)
  int kind = 0;                 // the owning engine's pack enum
  void* dst = nullptr;          // destination, or the hi half of a split pair
  void* dst_lo = nullptr;       // the lo half / f16 rounding residual of the packed weight, or nullptr
  int rows = 0, cols = 0;       // source [rows][cols] of a transposing pack (cout / cin of a VAE convolution)
  int group = -1;               // slots of one group fill the same destination (a tied embedding): one loaded member satisfies all
  bool optional = false;        // accepted with any size and ignored; not required by check_loaded
  bool loaded = false;
};

// Slots in the order they were added: *_key(i) is what the Python loaders iterate.
class WeightSlots {
 public:
  WeightSlot& add(const std::string& key, int64_t numel, int kind, void* dst, int rows = 0, int cols = 0);
  WeightSlot& back() { return slots_.back(); }
  int size() const { return (int)slots_.size(); }
  const char* key(int i) const { return i >= 0 && i < size() ? slots_[i].key.c_str() : nullptr; }
  int alloc_stage(DeviceArena& arena, bool zero) { return arena.alloc(&stage_, (size_t)stage_numel_, zero); }   // after the last add
  // a key the engine does not have: LATTE_ERR_INVALID, "<who>: ..." naming it
  int find(const char* who, const char* key, WeightSlot** out);
  // The frame of a *_load_tensor call in front of the engine's `switch (slot.kind)`: key lookup, numel check
  // ("<who>: ... got N, expected M"; not for an optional slot, which is marked loaded here and needs nothing else), and a host
  // source copied into the staging buffer on `st`.  *src is what the pack kernels read.
  int begin_load(const char* who, const char* key, const float* data, int64_t numel, bool on_device, hipStream_t st, WeightSlot** out,
                 const float** src);
  // ... and behind it: a host source's staging buffer is reused by the next call, so the stream is drained first
  int end_load(WeightSlot& s, bool on_device, hipStream_t st);
  int check_loaded() const;   // LATTE_ERR_STATE naming the first slot that is neither loaded, optional, nor covered by its group

 private:
  std::vector<WeightSlot> slots_;
  std::map<std::string, int> index_;
  int64_t stage_numel_ = 0;
  float* stage_ = nullptr;
};

}  // namespace latte
