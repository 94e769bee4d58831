// dev_owner_host.cpp — DevOwner (ilswiss_amd/csrc/dev_owner.h) on the host, against stubs of the layer below it: a ctx whose "device memory" is
// malloc, counted block by block, and whose N-th allocation can be told to fail.  tests/test_dev_owner_host.py drives it through the C entry
// points at the end.
#include <cstdarg>
#include <cstdlib>
#include <set>

#include "../../ilswiss_amd/csrc/dev_owner.h"

struct ilsx_ctx {
  std::set<void*> live;
  int allocs_made = 0, fail_at = 0;   // fail_at: the 1-based allocation that fails (0 = none)
};

void ilsx_set_err(const char*, ...) {}
int ctx_alloc(ilsx_ctx* c, size_t bytes, void** out, bool zero) {
  if (++c->allocs_made == c->fail_at) return ILSX_ERR_NOMEM;
  void* p = zero ? calloc(1, bytes ? bytes : 16) : malloc(bytes ? bytes : 16);
  if (!p) return ILSX_ERR_NOMEM;
  c->live.insert(p);
  *out = p;
  return ILSX_OK;
}
int ctx_free(ilsx_ctx* c, void* p) {
  if (!p) return ILSX_OK;
  if (!c->live.erase(p)) return ILSX_ERR_ARG;
  free(p);
  return ILSX_OK;
}

extern "C" {
ilsx_ctx* doh_ctx_create() { return new ilsx_ctx(); }
void doh_ctx_destroy(ilsx_ctx* c) { for (void* p : c->live) free(p); delete c; }
int doh_ctx_live(ilsx_ctx* c) { return (int)c->live.size(); }
void doh_ctx_fail_at(ilsx_ctx* c, int nth) { c->fail_at = nth; c->allocs_made = 0; }

DevOwner* doh_owner_create(ilsx_ctx* c) { DevOwner* o = new DevOwner(); o->ctx = c; return o; }
void doh_owner_destroy(DevOwner* o) { delete o; }
int doh_owner_blocks(DevOwner* o) { return (int)o->blocks.size(); }
int doh_alloc(DevOwner* o, size_t count, float** out) { return o->alloc(out, count); }
int doh_free(DevOwner* o, void* p) { return o->free(p); }
void doh_release(DevOwner* o) { o->release(); }
int doh_dw_region(DevOwner* o, const float* g_lo, size_t span, size_t bytes, void** out) { return o->dw_region(g_lo, span, bytes, out); }
// a slab of three buffers (n0 floats | n1 doubles | n2 bytes) through the owner: their offsets from the base, -1 on failure
int doh_commit3(DevOwner* o, size_t n0, size_t n1, size_t n2, void** base, long long* offs) {
  float* a = nullptr; double* b = nullptr; char* c = nullptr;
  Slab s;
  s.add(&a, n0); s.add(&b, n1); s.add(&c, n2);
  int rc = o->commit(s, base);
  if (rc != ILSX_OK) return rc;
  offs[0] = (char*)a - (char*)*base; offs[1] = (char*)b - (char*)*base; offs[2] = c - (char*)*base; offs[3] = (long long)s.bytes;
  return ILSX_OK;
}
}
