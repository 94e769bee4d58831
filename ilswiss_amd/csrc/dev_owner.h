// dev_owner.h — the one owner of a handle's device allocations ("the library owns what *_create returned until *_destroy").
// Host-only: needs nothing from HIP beyond the two declarations below, so a host harness compiles it against stubs.
#pragma once
#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

#include "../../include/ilsx.h"

void ilsx_set_err(const char* fmt, ...);
// the layer below: ilsx_ctx::allocs (what ilsx_debug_ctx_allocs counts)
int ctx_alloc(ilsx_ctx* c, size_t bytes, void** out, bool zero = true);
int ctx_free(ilsx_ctx* c, void* p);   // waits for the ctx stream first

// One allocation carved into many buffers.  Every buffer an agent touches in a step then sits in ONE virtually contiguous
// range (a handful of 2 MiB translation fragments) instead of ~60 separate hipMalloc's: a kernel that reads a dozen of them
// as its first operands otherwise pays a dozen page-table walks before its first useful byte (measured: the first operands of
// the backward launch landed 2.5 us after workgroup start, the weights — one allocation — after 0.55 us).
struct Slab {
  std::vector<std::pair<void**, size_t>> items;
  size_t bytes = 0;
  template <class T> void add(T** p, size_t count) {
    bytes = (bytes + 255) & ~(size_t)255;
    items.push_back({(void**)p, bytes});
    bytes += count * sizeof(T);
  }
};

// Every handle with device memory holds one: create and the lazy paths allocate through it, destroy is release().
struct DevOwner {
  ilsx_ctx* ctx = nullptr;
  std::vector<void*> blocks;
  // row-range scratch of split weight-gradient launches (launch_bwd_dw): ONE region per gradient arena and layout, keyed by the table's
  // gradient range.  The kernels write only the live words of a region and rely on the padding words staying zero — true as long as no table
  // with another layout ever writes the same region, which is why a region lives and dies with the object whose gradients it serves
  struct DwRegion { const float* g_lo; size_t span; void* p; size_t bytes; };
  std::vector<DwRegion> dw;

  template <class T> int alloc_bytes(T** out, size_t bytes, bool zero = true) {
    int rc = ctx_alloc(ctx, bytes, (void**)out, zero);
    if (rc == ILSX_OK) blocks.push_back(*out);
    return rc;
  }
  template <class T> int alloc(T** out, size_t count, bool zero = true) { return alloc_bytes(out, count * sizeof(T), zero); }
  int commit(Slab& s, void** base) {   // zero-filled
    int rc = alloc_bytes(base, s.bytes ? s.bytes : 256, true);
    if (rc != ILSX_OK) return rc;
    for (auto& it : s.items) *it.first = (char*)*base + it.second;
    return ILSX_OK;
  }
  int free(void* p) {
    if (!p) return ILSX_OK;
    auto it = std::find(blocks.begin(), blocks.end(), p);
    if (it == blocks.end()) { ilsx_set_err("DevOwner::free: pointer not owned by this object"); return ILSX_ERR_ARG; }
    blocks.erase(it);
    return ctx_free(ctx, p);
  }
  // the zero-filled region of the gradient range [g_lo, g_lo + span), grown to `bytes`
  int dw_region(const float* g_lo, size_t span, size_t bytes, void** out) {
    DwRegion* reg = nullptr;
    for (auto& r : dw) if (r.g_lo == g_lo && r.span == span) reg = &r;
    if (!reg) { dw.push_back({g_lo, span, nullptr, 0}); reg = &dw.back(); }
    if (reg->bytes < bytes) {
      int rc = free(reg->p);
      reg->p = nullptr; reg->bytes = 0;
      if (rc == ILSX_OK) rc = alloc_bytes(&reg->p, bytes, true);
      if (rc != ILSX_OK) return rc;
      reg->bytes = bytes;
    }
    *out = reg->p;
    return ILSX_OK;
  }
  void release() {   // idempotent
    for (void* p : blocks) ctx_free(ctx, p);
    blocks.clear();
    dw.clear();
  }
};
