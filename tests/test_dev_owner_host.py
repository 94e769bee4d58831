"""CPU suite: DevOwner (ilswiss_amd/csrc/dev_owner.h), the one owner of a handle's device allocations, compiled for the host against stubs of
ctx_alloc / ctx_free that count live blocks and can fail the N-th allocation (tests/harness/dev_owner_host.cpp).  What every *_destroy and
every failing *_create of the library relies on: release() gives back exactly what the owner allocated, whatever happened before."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_NOMEM = 0, -1, -3   # include/ilsx.h


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="doh_")
    so = os.path.join(d, "libdoh.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-Wno-comment",
                           os.path.join(ROOT, "tests", "harness", "dev_owner_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    vp, pvp = C.c_void_p, C.POINTER(C.c_void_p)
    for name, res, args in (("doh_ctx_create", vp, []), ("doh_ctx_destroy", None, [vp]), ("doh_ctx_live", C.c_int, [vp]),
                            ("doh_ctx_fail_at", None, [vp, C.c_int]), ("doh_owner_create", vp, [vp]), ("doh_owner_destroy", None, [vp]),
                            ("doh_owner_blocks", C.c_int, [vp]), ("doh_alloc", C.c_int, [vp, C.c_size_t, pvp]),
                            ("doh_free", C.c_int, [vp, vp]), ("doh_release", None, [vp]),
                            ("doh_dw_region", C.c_int, [vp, vp, C.c_size_t, C.c_size_t, pvp]),
                            ("doh_commit3", C.c_int, [vp, C.c_size_t, C.c_size_t, C.c_size_t, pvp, C.POINTER(C.c_longlong)])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


@pytest.fixture
def ctx(lib):
    c = lib.doh_ctx_create()
    yield c
    lib.doh_ctx_destroy(c)


def _alloc(lib, owner, count=8):
    p = C.c_void_p()
    assert lib.doh_alloc(owner, count, C.byref(p)) == OK and p.value
    return p


def test_release_gives_everything_back_and_is_idempotent(lib, ctx):
    o = lib.doh_owner_create(ctx)
    lib.doh_release(o)                                   # an owner that never allocated
    assert lib.doh_ctx_live(ctx) == 0
    ptrs = [_alloc(lib, o, n).value for n in (1, 100, 0)]   # a zero-size request is a block like any other
    assert len(set(ptrs)) == 3 and lib.doh_ctx_live(ctx) == 3 and lib.doh_owner_blocks(o) == 3
    lib.doh_release(o)
    assert lib.doh_ctx_live(ctx) == 0 and lib.doh_owner_blocks(o) == 0
    lib.doh_release(o)
    assert lib.doh_ctx_live(ctx) == 0
    _alloc(lib, o)                                       # usable again after a release
    assert lib.doh_ctx_live(ctx) == 1
    lib.doh_release(o)
    assert lib.doh_ctx_live(ctx) == 0
    lib.doh_owner_destroy(o)


def test_alloc_is_zero_filled(lib, ctx):
    o = lib.doh_owner_create(ctx)
    p = _alloc(lib, o, 64)
    assert bytes(C.string_at(p, 64 * 4)) == bytes(64 * 4)
    lib.doh_release(o)
    lib.doh_owner_destroy(o)


def test_free_of_an_owned_pointer(lib, ctx):
    o = lib.doh_owner_create(ctx)
    a, b = _alloc(lib, o), _alloc(lib, o)
    assert lib.doh_free(o, a) == OK
    assert lib.doh_ctx_live(ctx) == 1 and lib.doh_owner_blocks(o) == 1
    assert lib.doh_free(o, a) == ERR_ARG                 # forgotten: a second free is refused
    assert lib.doh_free(o, None) == OK                   # NULL: nothing to do
    assert lib.doh_ctx_live(ctx) == 1
    lib.doh_release(o)                                   # frees b only
    assert lib.doh_ctx_live(ctx) == 0
    del b
    lib.doh_owner_destroy(o)


def test_free_of_a_foreign_pointer_is_an_error_and_frees_nothing(lib, ctx):
    o1, o2 = lib.doh_owner_create(ctx), lib.doh_owner_create(ctx)
    a, b = _alloc(lib, o1), _alloc(lib, o2)
    assert lib.doh_free(o1, b) == ERR_ARG
    assert lib.doh_ctx_live(ctx) == 2 and lib.doh_owner_blocks(o1) == 1 and lib.doh_owner_blocks(o2) == 1
    assert lib.doh_free(o2, b) == OK and lib.doh_free(o1, a) == OK
    assert lib.doh_ctx_live(ctx) == 0
    for o in (o1, o2):
        lib.doh_owner_destroy(o)


def test_a_slab_is_one_block(lib, ctx):
    o = lib.doh_owner_create(ctx)
    base, offs = C.c_void_p(), (C.c_longlong * 4)()
    assert lib.doh_commit3(o, 3, 5, 7, C.byref(base), offs) == OK
    assert lib.doh_ctx_live(ctx) == 1 and lib.doh_owner_blocks(o) == 1
    assert list(offs) == [0, 256, 512, 512 + 7]          # Slab's carving: every buffer on a 256-byte boundary, in the order added
    assert bytes(C.string_at(base, offs[3])) == bytes(offs[3])   # zero-filled
    assert lib.doh_commit3(o, 0, 0, 0, C.byref(base), offs) == OK   # an empty slab is still a block
    assert lib.doh_ctx_live(ctx) == 2
    lib.doh_release(o)
    assert lib.doh_ctx_live(ctx) == 0
    lib.doh_owner_destroy(o)


@pytest.mark.parametrize("slab_fails", [False, True])
def test_a_failed_allocation_leaves_nothing_after_release(lib, ctx, slab_fails):
    o = lib.doh_owner_create(ctx)
    lib.doh_ctx_fail_at(ctx, 3)
    _alloc(lib, o), _alloc(lib, o)
    p, offs = C.c_void_p(), (C.c_longlong * 4)()
    rc = lib.doh_commit3(o, 1, 1, 1, C.byref(p), offs) if slab_fails else lib.doh_alloc(o, 8, C.byref(p))
    assert rc == ERR_NOMEM and not p.value
    assert lib.doh_ctx_live(ctx) == 2 and lib.doh_owner_blocks(o) == 2   # the failed request is not on the list
    _alloc(lib, o)                                       # the fourth succeeds
    lib.doh_release(o)
    assert lib.doh_ctx_live(ctx) == 0
    lib.doh_owner_destroy(o)


def test_two_owners_release_independently(lib, ctx):
    o1, o2 = lib.doh_owner_create(ctx), lib.doh_owner_create(ctx)
    for _ in range(3):
        _alloc(lib, o1)
    for _ in range(2):
        _alloc(lib, o2)
    assert lib.doh_ctx_live(ctx) == 5
    lib.doh_release(o1)
    assert lib.doh_ctx_live(ctx) == 2 and lib.doh_owner_blocks(o2) == 2
    lib.doh_release(o1)
    assert lib.doh_ctx_live(ctx) == 2
    lib.doh_release(o2)
    assert lib.doh_ctx_live(ctx) == 0
    for o in (o1, o2):
        lib.doh_owner_destroy(o)


def test_scratch_regions_one_per_gradient_range_and_released_with_the_owner(lib, ctx):
    """launch_bwd_dw's row-range scratch: one zeroed region per (g_lo, span), grown when a launch needs more, gone with release()."""
    o = lib.doh_owner_create(ctx)
    G = (C.c_float * 64)()
    g0, g1 = C.addressof(G), C.addressof(G) + 32 * 4
    a, a2, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert lib.doh_dw_region(o, g0, 32, 1024, C.byref(a)) == OK
    assert lib.doh_dw_region(o, g0, 32, 512, C.byref(a2)) == OK and a2.value == a.value   # large enough: the same region
    assert lib.doh_ctx_live(ctx) == 1
    assert lib.doh_dw_region(o, g1, 32, 1024, C.byref(b)) == OK and b.value != a.value    # another arena
    assert lib.doh_dw_region(o, g0, 16, 1024, C.byref(c)) == OK and c.value not in (a.value, b.value)   # same arena, another layout
    assert lib.doh_ctx_live(ctx) == 3
    assert lib.doh_dw_region(o, g0, 32, 4096, C.byref(a2)) == OK   # grown: the old block goes, the new one is zeroed
    assert lib.doh_ctx_live(ctx) == 3 and bytes(C.string_at(a2, 4096)) == bytes(4096)
    lib.doh_ctx_fail_at(ctx, 1)
    assert lib.doh_dw_region(o, g1, 32, 8192, C.byref(b)) == ERR_NOMEM and lib.doh_ctx_live(ctx) == 2
    lib.doh_ctx_fail_at(ctx, 0)
    assert lib.doh_dw_region(o, g1, 32, 8192, C.byref(b)) == OK and lib.doh_ctx_live(ctx) == 3   # the region recovers
    lib.doh_release(o)
    assert lib.doh_ctx_live(ctx) == 0
    assert lib.doh_dw_region(o, g0, 32, 256, C.byref(a)) == OK and lib.doh_ctx_live(ctx) == 1    # no stale region survives a release
    lib.doh_release(o)
    assert lib.doh_ctx_live(ctx) == 0
    lib.doh_owner_destroy(o)
