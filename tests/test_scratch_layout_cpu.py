"""The scratch sizes the C ABI reports, pinned against the values the library returned before the layouts became single
walks (tests/golden/scratch_bytes.json, recorded from that earlier build), and the refusals of the matcher's and the flat
index's entry points that return before anything touches a device.  No GPU involved."""
import ctypes as C
import json
import os

import pytest

from conftest import GOLDEN
from nano_vs_slam_amd import _lib

with open(os.path.join(GOLDEN, "scratch_bytes.json")) as fh:
    CASES = json.load(fh)["cases"]
ARG, UNSUPPORTED, WORKSPACE = -1, -2, -5


@pytest.mark.parametrize("fn", sorted(CASES))
def test_scratch_sizes_are_what_they_were(fn):
    f = getattr(_lib.load(), fn)
    got = [[args, int(f(*args))] for args, _ in CASES[fn]]
    assert got == CASES[fn]


def _vpr_merge_levels(nq, ndb, dim, k):
    """vpr.hip's slicing restated: database slices of whole 128-row tiles, merged G lists at a time."""
    T, qb = -(-ndb // 128), -(-nq // 64)
    nz = max(1, min(-(-768 // qb), T, (1 << 28) // (nq * k * 8), 65535))
    nz = -(-T // -(-T // nz)) if T else 1
    G, levels = max(2, 2048 // k), 0
    while nz > 1:
        nz, levels = -(-nz // G), levels + 1
    return levels


def test_the_table_reaches_both_sides_of_every_branch():
    valid = {fn: [tuple(a) for a, b in rows if b > 0] for fn, rows in CASES.items()}
    for fn, rows in CASES.items():
        assert any(b == 0 for _, b in rows), fn                                # the zero-returning invalid arguments
    m = valid["kp2d_match_scratch_bytes"]
    assert {(2, 37, 53), (512, 8, 8), (1, 1000, 1000), (64, 1000, 1000)} <= set(m)
    assert {(min(m0, m1) + 63) // 64 * B < 512 for B, m0, m1 in m} == {True, False}      # with and without partial arrays
    v = valid["kp2d_vpr_scratch_bytes"]
    assert {0, 1, 2} <= {_vpr_merge_levels(*a) for a in v} and any(a[1] == 0 for a in v)
    k = valid["kp2d_kmeans_scratch_bytes"]
    assert any(n % 16384 == 0 for n, _, _ in k) and any(n % 16384 for n, _, _ in k)
    assert any((1 << 22) // kk < (n + 255) // 256 for n, _, kk in k)           # the histogram cap sets the slab count
    p = valid["kp2d_kp_scratch_bytes"]
    assert {0, 32, 128} <= {a[3] for a in p}
    assert any(a[4] < min(a[1], a[2]) for a in p) and any(a[4] > max(a[1], a[2]) for a in p)


def _fake(addr=4096):
    return C.c_void_p(addr)          # never dereferenced: every case below is refused by the argument checks


@pytest.fixture(scope="module")
def refused():
    lib = _lib.load()

    def check(rc, code, text):
        assert rc == code, (rc, lib.kp2d_last_error())
        assert text.encode() in lib.kp2d_last_error(), lib.kp2d_last_error()
        with pytest.raises(_lib.Kp2dError):
            _lib.check(rc)
    return check


def test_matcher_refusals_without_a_device(refused):
    lib = _lib.load()
    need = lib.kp2d_match_scratch_bytes(2, 37, 53)
    ok = dict(d0=_fake(), n0=_fake(), d1=_fake(), n1=_fake(), B=2, max0=37, max1=53, C=32, cls0=None, cls1=None, flags=0,
              nn_idx=_fake(), nn_dist=_fake(), nn_dist2=_fake(), match_q=_fake(), match_d=_fake(), scratch=_fake(), nbytes=need)

    def ex(**kw):
        a = dict(ok, **kw)
        return lib.kp2d_match_descriptors_ex(a["d0"], a["n0"], a["d1"], a["n1"], a["B"], a["max0"], a["max1"], a["C"], 0.7,
                                             a["cls0"], a["cls1"], a["flags"], a["nn_idx"], a["nn_dist"], a["nn_dist2"],
                                             a["match_q"], a["match_d"], a["scratch"], a["nbytes"], None)

    def plain(**kw):
        a = dict(ok, **kw)
        return lib.kp2d_match_descriptors(a["d0"], a["n0"], a["d1"], a["n1"], a["B"], a["max0"], a["max1"], a["C"], 0.7,
                                          a["nn_idx"], a["nn_dist"], a["nn_dist2"], a["match_q"], a["match_d"], a["scratch"], None)

    for name in ("d0", "n0", "d1", "n1", "nn_idx", "nn_dist", "nn_dist2", "match_q", "match_d", "scratch"):
        refused(ex(**{name: None}), ARG, "null argument")
        refused(plain(**{name: None}), ARG, "null argument")
    for kw in (dict(B=0), dict(max0=0), dict(max1=-1)):
        refused(ex(**kw), ARG, "empty match problem")
        refused(plain(**kw), ARG, "empty match problem")
    refused(ex(cls0=_fake()), ARG, "class ids must be given for both sides or neither")
    refused(ex(cls1=_fake()), ARG, "class ids must be given for both sides or neither")
    refused(ex(flags=2), ARG, "unknown match flags 0x2")
    # a short scratch: the refusal names the size kp2d_match_scratch_bytes answers, whatever part of it the call could do without
    base = 2 * 53 * 16
    assert base < need
    for nbytes in (0, base - 1):
        refused(ex(nbytes=nbytes), WORKSPACE, f"match scratch {nbytes} B < required {need} B (kp2d_match_scratch_bytes)")
    refused(ex(scratch=_fake(4100)), WORKSPACE, "match scratch must be 8-byte aligned")
    refused(ex(scratch=_fake(4100), nbytes=base), WORKSPACE, "match scratch must be 8-byte aligned")   # (degraded size: accepted)

    pok = dict(match_q=_fake(), match_d=_fake(), pts0=_fake(), pts1=_fake(), B=2, max0=37, max1=53, pairs=_fake(), idx=_fake(),
               dist=_fake(), count=_fake())

    def pairs(**kw):
        a = dict(pok, **kw)
        return lib.kp2d_match_pairs(a["match_q"], a["match_d"], a["pts0"], a["pts1"], a["B"], a["max0"], a["max1"], a["pairs"],
                                    a["idx"], a["dist"], a["count"], None)

    for kw in (dict(match_q=None), dict(count=None), dict(match_d=None), dict(pts0=None), dict(pts1=None)):
        refused(pairs(**kw), ARG, "null argument")
    refused(pairs(B=0), ARG, "empty match problem")

    tneed = lib.kp2d_match_topk_scratch_bytes(2, 37, 53)
    tok = dict(mode=0, match_q=_fake(), matches0=_fake(), val=_fake(), pts0=_fake(), pts1=_fake(), B=2, max0=37, max1=53, k=10,
               pairs=_fake(), idx=_fake(), out_val=_fake(), count=_fake(), scratch=_fake(), nbytes=tneed)

    def topk(**kw):
        a = dict(tok, **kw)
        return lib.kp2d_match_topk_pairs(a["mode"], a["match_q"], a["matches0"], a["val"], a["pts0"], a["pts1"], a["B"], a["max0"],
                                         a["max1"], a["k"], a["pairs"], a["idx"], a["out_val"], a["count"], a["scratch"],
                                         a["nbytes"], None)

    refused(topk(mode=2), ARG, "mode is KP2D_TOPK_BF or KP2D_TOPK_LG")
    for kw in (dict(val=None), dict(count=None), dict(scratch=None), dict(match_q=None), dict(mode=1, matches0=None),
               dict(pts0=None), dict(pts1=None)):
        refused(topk(**kw), ARG, "null argument")
    refused(topk(max0=0), ARG, "empty match problem")
    for mode in (0, 1):                              # the size does not depend on the mode: max(max0, max1) rows
        refused(topk(mode=mode, nbytes=tneed - 1), WORKSPACE, "match top-k scratch too small")
    refused(topk(scratch=_fake(4098)), ARG, "match top-k scratch must be 4-byte aligned")


def test_vpr_refusals_without_a_device(refused):
    lib = _lib.load()

    def pack(x=_fake(), n=10, dim=32, packed=_fake()):
        return lib.kp2d_vpr_pack(x, n, dim, packed, None)

    for dim in (8, 40, 16400):
        refused(pack(dim=dim), UNSUPPORTED, f"vpr: descriptor dim {dim} (needs dim % 16 == 0, 16 <= dim <= 16384)")
    refused(pack(n=-1), ARG, "vpr_pack: row count -1")
    refused(pack(n=2 ** 31), ARG, f"vpr_pack: row count {2 ** 31}")
    assert pack(n=0, x=None, packed=None) == 0
    refused(pack(x=None), ARG, "null argument")
    refused(pack(packed=None), ARG, "null argument")
    refused(pack(x=_fake(4104)), ARG, "vpr_pack: x and packed must be 16-byte aligned")

    need = lib.kp2d_vpr_scratch_bytes(3, 3000, 32, 5)
    ok = dict(packed=_fake(), db=_fake(), ndb=3000, dim=32, q=_fake(), nq=3, limit=None, k=5, flags=0, dist=_fake(), idx=_fake(),
              scratch=_fake(), nbytes=need)

    def search(**kw):
        a = dict(ok, **kw)
        return lib.kp2d_vpr_search(a["packed"], a["db"], a["ndb"], a["dim"], a["q"], a["nq"], a["limit"], a["k"], a["flags"],
                                   a["dist"], a["idx"], a["scratch"], a["nbytes"], None)

    refused(search(dim=24), UNSUPPORTED, "vpr: descriptor dim 24")
    refused(search(k=0), ARG, "vpr_search: k = 0 outside [1, 1024]")
    refused(search(k=1025), ARG, "vpr_search: k = 1025 outside [1, 1024]")
    refused(search(nq=-1), ARG, "vpr_search: negative size")
    refused(search(ndb=-1), ARG, "vpr_search: negative size")
    refused(search(ndb=2 ** 31), UNSUPPORTED, "vpr_search: more than 2^31 - 1 database rows")
    refused(search(flags=2), ARG, "unknown vpr flags 0x2")
    assert search(nq=0, q=None, scratch=None) == 0
    for name in ("q", "dist", "idx", "scratch", "packed", "db"):
        refused(search(**{name: None}), ARG, "null argument")
    assert search(ndb=0, packed=None, db=None, nbytes=0) == WORKSPACE          # (an empty database needs no database pointers)
    for name in ("q", "db", "packed", "scratch"):
        refused(search(**{name: _fake(4104)}), ARG, "vpr_search: q, db, packed_db and scratch must be 16-byte aligned")
    for nbytes in (0, need - 1):
        refused(search(nbytes=nbytes), WORKSPACE, f"vpr scratch {nbytes} B < required {need} B (kp2d_vpr_scratch_bytes)")
