"""Host-integer plan of the segmented cross-attention (a batch of different videos decoded together): vidi_amd/shard.py
`plan_cross_segments` against the rules csrc/attn_cross_seg.hip relies on, and the C ABI's two new entry points.  No GPU."""
import itertools
import os
import re

import pytest

from vidi_amd.shard import XSEG_REC, CrossSegment, plan_cross_segments, share_key_slices, single_key_slices, split_key_slices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG = (0, 17, 333, 11250, 90000)
AUD = (0, 100, 4500)
TOK = (1, 7, 16, 17, 39, 52)
SHAPES = ((8, 2, 256), (2, 4, 128))          # (nkv, G, HD): Vidi1.5-9B and the HD 128 / G 4 shape of the kernel tests


def r64(x):
    return (x + 63) // 64 * 64


def make_segments(imgs, auds, toks, masked=()):
    segs, tok0, key0 = [], 0, 0
    for i, (ni, na, nt) in enumerate(zip(imgs, auds, toks)):
        a0 = key0 + r64(ni)
        segs.append(CrossSegment(tok0=tok0, ntok=nt, img_start=key0, n_img=ni, img_mask=key0 if i in masked else -1,
                                 aud_start=a0, n_aud=na, aud_mask=-1))
        tok0 += nt
        key0 = a0 + r64(na)
    return segs


def sweep():
    """1-8 videos; every key count and prompt length of the issue's lists appears, alone and mixed"""
    cases = []
    for n in range(1, 9):
        for k, (ni, na, nt) in enumerate(itertools.product(IMG, AUD, TOK)):
            if n > 1 and k % n:              # thin the product for the larger batches (every value still occurs at every batch size)
                continue
            imgs = [IMG[(IMG.index(ni) + j) % len(IMG)] for j in range(n)]
            auds = [AUD[(AUD.index(na) + j) % len(AUD)] for j in range(n)]
            toks = [TOK[(TOK.index(nt) + 2 * j) % len(TOK)] for j in range(n)]
            cases.append((imgs, auds, toks))
        cases.append(([ni for ni in IMG[:n]] + [90000] * max(0, n - len(IMG)), [4500] * n, [52] * n))
    return cases


def check_plan(segs, nkv, G, HD, budget=256):
    plan = plan_cross_segments(segs, nkv, G, HD, budget)
    cover = {}                                # (segment, modality, row tile) -> sub-tile -> owners
    regions = []
    for it in plan.items:
        assert len(it) == XSEG_REC
        tok0, R, rt, ks, nk, moff, z, zs, base, Rpad, one = it[:11]
        si = [i for i, s in enumerate(segs) if s.tok0 == tok0][0]
        s = segs[si]
        mod = 0 if (ks, nk) == (s.img_start, s.n_img) and s.n_img else 1
        assert (ks, nk) == ((s.img_start, s.n_img) if mod == 0 else (s.aud_start, s.n_aud)) and nk > 0 and ks % 64 == 0
        assert R == s.ntok * G and Rpad == (R + 31) // 32 * 32 and 0 <= rt < Rpad // 32 and one == int(Rpad == 32)
        assert zs == plan.zsplit[si][mod] >= 1 and 0 <= z < zs
        assert moff == (s.img_mask if mod == 0 else s.aud_mask)
        nsub = (nk + 31) // 32
        # the kernel's interleave rule: wave wg = z * 4 + w of the pair's zs * 4 waves sweeps sub-tiles wg, wg + 4 zs, ...
        tiles = cover.setdefault((si, mod, rt), {})
        for w in range(4):
            for st in range(z * 4 + w, nsub, 4 * zs):
                tiles.setdefault(st, []).append((z, w))
        regions.append((si, mod, base, zs * nkv * Rpad))
    for si, s in enumerate(segs):
        R = s.ntok * G
        for mod, n in ((0, s.n_img), (1, s.n_aud)):
            if n == 0:
                assert plan.zsplit[si][mod] == 0
                continue
            nsub = (n + 31) // 32
            zs = plan.zsplit[si][mod]
            assert zs >= 1
            # the engine's rule for "no slice shorter than 8 sub-tiles unless the pair is" (shard.single_key_slices, split_key_slices): never
            # more slices than the region has runs of 8 sub-tiles
            assert zs <= (nsub + 7) // 8
            for rt in range((R + 31) // 32):
                tiles = cover[(si, mod, rt)]
                assert sorted(tiles) == list(range(nsub)) and all(len(o) == 1 for o in tiles.values())
    # partial regions: disjoint, inside the workspace, and the segment table names the same ones
    uniq = sorted(set(regions), key=lambda r: r[2])
    end = 0
    for si, mod, base, rows in uniq:
        assert base >= end
        end = base + rows
        rec = plan.segs[si]
        assert rec[3 + 3 * mod] == base and rec[4 + 3 * mod] == plan.zsplit[si][mod]
    assert end <= plan.part_rows
    assert plan.workspace_floats(HD) == (plan.part_rows * HD, plan.part_rows * 2)
    for si, s in enumerate(segs):
        rec = plan.segs[si]
        assert rec[:3] == [s.tok0, s.ntok * G, (s.ntok * G + 31) // 32 * 32] and len(rec) == XSEG_REC
    # blocks per launch <= budget; the launches tile the item list; a single launch whenever one slice per pair and row tile fits
    assert sum(c for _, c in plan.launches) == len(plan.items) and [a for a, _ in plan.launches] == \
        [sum(c for _, c in plan.launches[:i]) for i in range(len(plan.launches))]
    for _, c in plan.launches:
        assert c * nkv <= budget
    min_items = sum(((s.ntok * G + 31) // 32) * (int(s.n_img > 0) + int(s.n_aud > 0)) for s in segs)
    if min_items * nkv <= budget:
        assert len(plan.launches) <= 1
    # longest slice first
    def longest(it):
        nsub, z, zs = (it[4] + 31) // 32, it[6], it[7]
        return len(range(z * 4, nsub, 4 * zs))
    ls = [longest(it) for it in plan.items]
    assert ls == sorted(ls, reverse=True)
    assert plan.max_rows == max(s.ntok for s in segs) * G
    assert len(plan.launch_keys) == len(plan.launches) and abs(sum(plan.launch_keys) - sum(s.n_img + s.n_aud for s in segs)) <= len(plan.launches)
    return plan


@pytest.mark.parametrize("nkv,G,HD", SHAPES)
def test_plan_invariants_over_the_sweep(nkv, G, HD):
    n = 0
    for imgs, auds, toks in sweep():
        check_plan(make_segments(imgs, auds, toks, masked=(0,)), nkv, G, HD)
        n += 1
    assert n > 100


@pytest.mark.parametrize("nkv,G,HD", SHAPES)
def test_one_segment_reproduces_the_one_video_zsplit(nkv, G, HD):
    """The expectation is the engine's own code: `VidiEngine._cross_local` sizes one modality with `shard.single_key_slices(256 // (nkv x row
    blocks), sub-tiles)`, `_cross_dual` two with `split_key_slices`, and both take the row blocks from the library
    (`vidi_attn_cross_row_tiles_per_block`).  For a single row tile (decode, prompts up to 32 / G tokens) the library's answer is one block
    per tile and the plan must give exactly the one-video values.  From two row tiles on the one-video launch switches to the shared-stream
    kernel (4 row tiles per block); the segmented launch stays on the per-tile kernel in this version, so there the expectation is the
    same code at one block per row tile."""
    import torch
    from vidi_amd import hip
    hip.load_library()
    for ni, na, nt in itertools.product(IMG, AUD, TOK):
        if ni == 0 and na == 0:
            continue
        plan = check_plan(make_segments([ni], [na], [nt]), nkv, G, HD)
        Rpad = (nt * G + 31) // 32 * 32
        rtpb = hip.attn_cross_row_tiles_per_block(Rpad, 50.0, torch.bfloat16) if Rpad == 32 else 1
        assert rtpb == 1
        row_blocks = -(-(Rpad // 32) // rtpb)
        Z = 256 // max(1, nkv * row_blocks)
        si, sa = (ni + 31) // 32, (na + 31) // 32
        if ni and na:
            assert Z >= 2
            want = split_key_slices(Z, si, sa)                                           # engine.py `_cross_dual`
        else:
            want = tuple(single_key_slices(Z, s) if s else 0 for s in (si, sa))          # engine.py `_cross_local`
        assert plan.zsplit[0] == want, (ni, na, nt, plan.zsplit, want)
    assert (single_key_slices(32, 352), single_key_slices(32, 20), single_key_slices(0, 5), single_key_slices(32, 9)) == (32, 3, 1, 2)


def test_two_regions_reproduce_split_key_slices():
    for Z in (2, 3, 8, 16, 31, 32, 128):
        for a, b in itertools.product((1, 2, 11, 141, 352, 2813), repeat=2):
            assert tuple(share_key_slices(Z, [a, b])) == split_key_slices(Z, a, b), (Z, a, b)
    assert share_key_slices(32, [352]) == [32] and share_key_slices(32, [20]) == [3] and share_key_slices(4, [1, 1, 1, 1]) == [1, 1, 1, 1]
    with pytest.raises(ValueError):
        share_key_slices(1, [5, 5])


def test_plan_rejects_bad_segments():
    with pytest.raises(ValueError):
        plan_cross_segments([], 8, 2, 256)
    with pytest.raises(ValueError):
        plan_cross_segments([CrossSegment(0, 1, img_start=32, n_img=10)], 8, 2, 256)
    with pytest.raises(ValueError):
        plan_cross_segments([CrossSegment(0, 0, n_img=10)], 8, 2, 256)
    with pytest.raises(ValueError):
        plan_cross_segments([CrossSegment(0, 1, n_img=10)], 8, 2, 64)


def test_abi_6_declares_and_binds_the_segment_entry_points():
    from vidi_amd import hip
    src = open(os.path.join(ROOT, "include", "vidi_hip.h")).read()
    assert re.search(r"#define VIDI_ABI_VERSION 6\b", src)
    for name in ("vidi_attn_cross_seg", "vidi_attn_merge_seg"):
        assert name in hip.SIGNATURES
        assert re.search(r"\bint " + name + r"\(", src)
    import __graft_entry__ as GE
    assert GE.header_abi_version() == 6


def test_segment_entry_points_validate_before_any_launch():
    """null pointers, a head dim the kernels do not have and an empty table are refused with negative codes (no GPU needed)"""
    import ctypes
    from vidi_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    ll, vp = ctypes.c_longlong, ctypes.c_void_p
    lib.vidi_abi_version.restype = ctypes.c_int
    assert lib.vidi_abi_version() == 6
    buf = (ctypes.c_int * 64)()
    ptr = ctypes.cast(buf, vp)
    f = ctypes.c_float
    cross = lambda q, items, n_items, HD: lib.vidi_attn_cross_seg(q, ptr, ptr, None, ll(0), ptr, ptr, ll(1024), items, n_items, 4, 2, 8, HD, 4608,  # noqa: E731
                                                                 16, f(0.0625), f(50.0), 0, None)
    assert cross(None, ptr, 1, 256) == -4
    assert cross(ptr, None, 1, 256) == -4
    assert cross(ptr, ptr, 0, 256) == -1
    assert cross(ptr, ptr, 1, 64) == -1
    merge = lambda op, segs, n, out, HD: lib.vidi_attn_merge_seg(op, ptr, ll(1024), segs, n, 2, out, None, 4, 8, 2, HD, 4096, 0, None)   # noqa: E731
    assert merge(None, ptr, 1, ptr, 256) == -4
    assert merge(ptr, None, 1, ptr, 256) == -4
    assert merge(ptr, ptr, 1, None, 256) == -4
    assert merge(ptr, ptr, 0, ptr, 256) == -1
    assert merge(ptr, ptr, 1, ptr, 96) == -1
