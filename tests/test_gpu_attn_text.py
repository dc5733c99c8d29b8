"""The text (T2T) attention kernels against a float64 reference at their loop edges.

Every T2T launch runs through `attn_text_kernel` (csrc/attn_text.hip: prefill, the k+1 rows of a speculative verify step, the
`vidi_attn_text_dyn` decode fallback) or `attn_text_decode_body` (csrc/attn_text_decode.h: `vidi_attn_text_decode`, `..._merge2`,
`..._rows`).  The other files compare these with each other; here both are held to `t2t_ref`, arithmetic that is not ours:

  1. `t2t_ref`: float64 on the CPU over inputs already rounded to the dtype; scores (K q) * scale with the optional softcap, invisible
     keys -inf, p = exp(s - max), the denominator over the unrounded p, p rounded to the dtype before p @ V (the formulation both
     kernels document and `O.sdpa_reference` uses), zeros for a row without a visible key.
  2. `vidi_attn_text` over (past, Lq) groups that straddle the scalar PV tail, the 16-row PV batch, the 64-key score pass, the second
     pass and 256 keys, each with window 0 / 16 / 40 and no / right-padding / left-padding key mask; q x 4; `vidi_attn_text_dyn`.
  3. the key census on the same launches: Q = 0 and one-hot V rows turn the output into a count of the visible keys per column, so one
     dropped, doubled or leaked key moves a column by >= 1 / n.
  4. the decode body through `vidi_attn_text_decode_rows` at 18 positions on both sides of its 64 / 128-key score steps, its 64-lane
     softmax stride and its PV stride, with G = 1, 2, 3, 4; then the masked form through `vidi_attn_text_decode`.
  5. `vidi_rope` / `vidi_rope_cache` against `O.apply_rope` evaluated in the model dtype, bit for bit.
  6. what `hip.attn_text` refuses.

Bound (sections 2 and 4), the project's rule:  |got - ref| <= atol + rtol * |ref|  with rtol = 1e-2 (bf16) / 2e-3 (fp16) and
atol = rtol * rms(reference row), the rms taken per (row, head) of the REFERENCE.  `check` divides both sides by that rms, so that one
`report` call with a scalar atol applies the per-row bound.  A CPU fp32 emulation of the kernels' formulation uses 0.28 (bf16) / 0.17
(fp16) of it; the kernels add `__expf`, `tanhf` and their summation order.

Census bound: the exact count / n rounded once to the dtype, |got - exact| <= u * |exact| with u = 2^-8 (bf16) / 2^-11 (fp16), plus
2^-19 relative for the fp32 count * (1 / n) in front of the rounding; columns without a visible key are bit-zero.

Worst `tol_used` per test on an MI355X (VIDI_TEST_REPORT, fraction of the bound; bf16 / fp16):
  test_attn_text_against_fp64                  0.41 / 0.25   (bf16: HD 64, 13 .. 20 keys, left padding — 1 .. 6 visible keys)
  test_attn_text_peaked_softmax_against_fp64   0.27 / 0.26
  test_attn_text_dyn_against_fp64              0.28 / 0.26
  test_decode_rows_against_fp64                0.28 / 0.18
  test_decode_masked_against_fp64              0.28 / 0.17
  test_attn_text_key_census                    0.99 / 0.83   (the census bound IS one rounding: a count / n next to a rounding tie uses all
  test_attn_text_dyn_key_census                0.66 / 0.72    of it; a wrong key would use >= 50 x the bound)
  test_decode_rows_key_census                  0.99 / 0.68
The kernels use what the fp32 emulation uses: `__expf`, `tanhf` and the summation order do not show at this resolution.

Section 5 found the fp16 rope off by an ulp in about one element in five: the compiler narrowed `rnd(x1 * c1) + rnd(-x2 * s1)` to half
arithmetic and contracted one product into the sum (v_fma_f16), so that product never rounded.  `rope_pair` (csrc/attn_text_decode.h) now
holds the three rope sites with contraction off; the bf16 code did not change.
"""
import pytest
import torch

import vidi_oracle as O
from util import report, seeded

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "fp16"]
SENTINEL = 7.0


@pytest.fixture(scope="module")
def hip():
    from vidi_amd import hip as h
    h.load_library()
    return h


def bits(t):
    return t.view(torch.int16)


def rtol_of(dt):
    return 1e-2 if dt == torch.bfloat16 else 2e-3


def unit_roundoff(dt):
    return 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the reference
# ---------------------------------------------------------------------------------------------------------------------------------------
def t2t_ref(q, K, V, visible, scale, softcap, dt):
    """q [B, R, nq, HD], K / V [B, L, nkv, HD] (values already rounded to `dt`), visible [B, R, L] bool -> [B, R, nq, HD] float64"""
    G = q.shape[2] // K.shape[2]
    q, K, V = q.double(), K.double().repeat_interleave(G, dim=2), V.double().repeat_interleave(G, dim=2)
    s = torch.einsum("brhd,blhd->brhl", q, K) * scale
    if softcap:
        s = softcap * torch.tanh(s / softcap)
    s = s.masked_fill(~visible[:, :, None, :], float("-inf"))
    mx = s.amax(dim=-1, keepdim=True)
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)                     # a row without a visible key: every p is 0
    p = torch.exp(s - mx)
    den = p.sum(dim=-1)                                                             # over the unrounded p
    num = torch.einsum("brhl,blhd->brhd", p.float().to(dt).double(), V)             # p in the dtype before PV
    return torch.where(den[..., None] > 0, num / den.clamp_min(1e-300)[..., None], torch.zeros_like(num))


def check(name, got, ref, dt):
    """got / ref [..., HD] with one (row, head) per leading index: the bound of the module docstring, the rms per (row, head) of the
    reference; a reference row of zeros (no visible key) must come back as zeros"""
    got, ref = got.detach().cpu(), ref.detach().cpu().double()
    assert torch.isfinite(got.float()).all(), f"{name}: non-finite output"
    rms = ref.pow(2).mean(dim=-1, keepdim=True).sqrt()
    dead = (rms == 0).expand_as(ref)
    assert bool((got[dead] == 0).all()), f"{name}: a row without a visible key is not zero"
    rms = torch.where(rms == 0, torch.ones_like(rms), rms)
    r = rtol_of(dt)
    return report(name, got.double() / rms, ref / rms, r, r)


def check_census(name, got, count, nvis, dt):
    """got [..., HD] against count / nvis (exact in float64), one rounding of the dtype away; columns without a key bit-zero"""
    got = got.detach().cpu()
    exact = torch.where(nvis > 0, count / nvis.clamp_min(1.0), torch.zeros_like(count))
    empty = exact == 0
    assert bool((bits(got)[empty] == 0).all()), f"{name}: a column without a visible key is not bit-zero"
    return report(name, got, exact, 0.0, unit_roundoff(dt) + 2.0 ** -19)


def one_hot_v(L, nkv, HD, dt, lead):
    """V[..., j, h, :] one-hot at column j % HD"""
    v = torch.zeros((L, HD))
    v[torch.arange(L), torch.arange(L) % HD] = 1.0
    return v[:, None, :].expand(L, nkv, HD).expand(*lead, L, nkv, HD).to(dt).contiguous()


def census_expect(visible, HD):
    """visible [..., L] bool -> (count [..., HD] of visible j with j % HD == d, number of visible keys [..., 1]), float64"""
    L = visible.shape[-1]
    col = torch.zeros((L, HD), dtype=torch.float64)
    col[torch.arange(L), torch.arange(L) % HD] = 1.0
    vis = visible.double()
    return vis @ col, vis.sum(dim=-1, keepdim=True)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. vidi_attn_text (prefill / verify form) and vidi_attn_text_dyn
# ---------------------------------------------------------------------------------------------------------------------------------------
B, LMAX_T = 2, 288
SHAPES_T = [(4, 2, 256, 50.0), (8, 2, 128, 0.0), (2, 2, 64, 50.0)]                   # Gemma G = 2, Mistral G = 4 (no softcap), G = 1
SHAPE_T_IDS = ["gemma-hd256-g2", "mistral-hd128-g4", "hd64-g1"]
# (past, Lq): n = past + i + 1 keys; scalar PV tail only / the 16-row PV batch / the 64-key score pass / the second pass and the 8th
# PV batch / a full 16-row verify step across 256
GROUPS = [(0, 5), (12, 8), (60, 8), (124, 8), (250, 16)]
WINDOWS_T = [0, 16, 40]
MASKS = ["none", "right", "left"]
DYN_PAST = [0, 63, 64, 128]


def key_mask(kind, past):
    if kind == "none":
        return None
    km = torch.ones((B, LMAX_T), dtype=torch.uint8)
    if kind == "right":                                     # a hole in batch row 1 (test_rope_and_attn_text's) and one just below `past`,
        km[1, 3:6] = 0                                      # which every window of the group still covers
        km[1, max(past - 3, 0): past] = 0
    else:                                                   # left padding: query rows 0 and 1 of batch row 1 see no key, row 2 only itself
        km[1, : past + 2] = 0
    return km


def visible_text(past, Lq, window, km):
    qi = past + torch.arange(Lq)[:, None]
    kj = torch.arange(LMAX_T)[None, :]
    vis = kj <= qi
    if window:
        vis = vis & (kj >= qi - window)
    vis = vis[None].expand(B, Lq, LMAX_T)
    return vis if km is None else vis & km[:, None, :].bool()


@pytest.fixture(scope="module")
def text_inputs():
    """per (dt, shape): q rows for the longest group and caches random over ALL of Lmax (a future or out-of-window key that leaks in
    changes the result) — computed once, on the CPU and the device, and left unchanged"""
    memo = {}

    def get(dt, nq, nkv, HD):
        key = (dt, nq, nkv, HD)
        if key not in memo:
            q = seeded((B, 16, nq, HD), 150, dtype=dt)
            kc = seeded((B, LMAX_T, nkv, HD), 151, dtype=dt)
            vc = seeded((B, LMAX_T, nkv, HD), 152, dtype=dt)
            memo[key] = (q, kc, vc, kc.reshape(B, LMAX_T, -1).cuda(), vc.reshape(B, LMAX_T, -1).cuda(),
                         one_hot_v(LMAX_T, nkv, HD, dt, (B,)).reshape(B, LMAX_T, -1).cuda())
        return memo[key]
    return get


def launch_text(hip, q, kcd, vcd, km, *, Lq, nq, nkv, HD, past, window, cap, dyn=False):
    """q [B, Lq, nq, HD] on the CPU -> the kernel's output [B, Lq, nq, HD] on the CPU; rows start as a sentinel"""
    out = torch.full((B * Lq, nq * HD), SENTINEL, dtype=q.dtype, device="cuda")
    kmd = None if km is None else km.cuda()
    kw = dict(B=B, Lq=Lq, Lmax=LMAX_T, nq=nq, nkv=nkv, HD=HD, window=window, scale=HD ** -0.5, softcap=cap)
    qd = q.reshape(B * Lq, nq * HD).contiguous().cuda()
    if dyn:
        hip.attn_text_dyn(qd, kcd, vcd, kmd, out, past_len_dev=torch.tensor([past], dtype=torch.int32, device="cuda"), **kw)
    else:
        hip.attn_text(qd, kcd, vcd, kmd, out, past_len=past, **kw)
    return out.cpu().view(B, Lq, nq, HD)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("nq,nkv,HD,cap", SHAPES_T, ids=SHAPE_T_IDS)
@pytest.mark.parametrize("past,Lq", GROUPS)
def test_attn_text_against_fp64(hip, text_inputs, dt, nq, nkv, HD, cap, past, Lq):
    q, kc, vc, kcd, vcd, _ = text_inputs(dt, nq, nkv, HD)
    q = q[:, :Lq].contiguous()
    for window in WINDOWS_T:
        for mask in MASKS:
            km = key_mask(mask, past)
            vis = visible_text(past, Lq, window, km)
            ref = t2t_ref(q, kc, vc, vis, HD ** -0.5, cap, dt)
            out = launch_text(hip, q, kcd, vcd, km, Lq=Lq, nq=nq, nkv=nkv, HD=HD, past=past, window=window, cap=cap)
            check(f"attn_text past {past} Lq {Lq} window {window} mask {mask}", out, ref, dt)
            if mask == "left":                              # rows 0 and 1 of batch row 1: no visible key -> exactly zero (check() asserted
                assert not vis[1, :2].any() and int(vis[1, 2].sum()) == 1            # it); row 2 sees only itself


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("nq,nkv,HD,cap", SHAPES_T, ids=SHAPE_T_IDS)
def test_attn_text_peaked_softmax_against_fp64(hip, text_inputs, dt, nq, nkv, HD, cap):
    """q x 4: scores spread ~ 4, a softmax dominated by a few keys among 125 .. 132"""
    past, Lq = 124, 8
    q, kc, vc, kcd, vcd, _ = text_inputs(dt, nq, nkv, HD)
    q = (q[:, :Lq].float() * 4.0).to(dt)                                              # x 4 is exact in both dtypes
    vis = visible_text(past, Lq, 0, None)
    ref = t2t_ref(q, kc, vc, vis, HD ** -0.5, cap, dt)
    out = launch_text(hip, q, kcd, vcd, None, Lq=Lq, nq=nq, nkv=nkv, HD=HD, past=past, window=0, cap=cap)
    check("attn_text q x 4", out, ref, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("nq,nkv,HD,cap", SHAPES_T, ids=SHAPE_T_IDS)
def test_attn_text_dyn_against_fp64(hip, text_inputs, dt, nq, nkv, HD, cap):
    """the decode fallback: Lq = 1 with the position in device memory"""
    q, kc, vc, kcd, vcd, _ = text_inputs(dt, nq, nkv, HD)
    q = q[:, :1].contiguous()
    for past in DYN_PAST:
        for window in WINDOWS_T:
            for mask in MASKS:
                km = key_mask(mask, past)
                vis = visible_text(past, 1, window, km)
                ref = t2t_ref(q, kc, vc, vis, HD ** -0.5, cap, dt)
                out = launch_text(hip, q, kcd, vcd, km, Lq=1, nq=nq, nkv=nkv, HD=HD, past=past, window=window, cap=cap, dyn=True)
                check(f"attn_text_dyn past {past} window {window} mask {mask}", out, ref, dt)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. key census
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("nq,nkv,HD,cap", SHAPES_T, ids=SHAPE_T_IDS)
@pytest.mark.parametrize("past,Lq", GROUPS)
def test_attn_text_key_census(hip, text_inputs, dt, nq, nkv, HD, cap, past, Lq):
    """Q = 0: every score 0, every P 1, the denominator the number of visible keys; V one-hot at j % HD over all of Lmax"""
    _, _, _, kcd, _, v1d = text_inputs(dt, nq, nkv, HD)
    q = torch.zeros((B, Lq, nq, HD), dtype=dt)
    for window in WINDOWS_T:
        for mask in MASKS:
            km = key_mask(mask, past)
            count, nvis = census_expect(visible_text(past, Lq, window, km), HD)
            out = launch_text(hip, q, kcd, v1d, km, Lq=Lq, nq=nq, nkv=nkv, HD=HD, past=past, window=window, cap=cap)
            check_census(f"census past {past} Lq {Lq} window {window} mask {mask}", out, count[:, :, None, :].expand(B, Lq, nq, HD),
                         nvis[:, :, None, :].expand(B, Lq, nq, 1), dt)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("nq,nkv,HD,cap", SHAPES_T, ids=SHAPE_T_IDS)
def test_attn_text_dyn_key_census(hip, text_inputs, dt, nq, nkv, HD, cap):
    _, _, _, kcd, _, v1d = text_inputs(dt, nq, nkv, HD)
    q = torch.zeros((B, 1, nq, HD), dtype=dt)
    for past in DYN_PAST:
        for window in WINDOWS_T:
            for mask in MASKS:
                km = key_mask(mask, past)
                count, nvis = census_expect(visible_text(past, 1, window, km), HD)
                out = launch_text(hip, q, kcd, v1d, km, Lq=1, nq=nq, nkv=nkv, HD=HD, past=past, window=window, cap=cap, dyn=True)
                check_census(f"census dyn past {past} window {window} mask {mask}", out, count[:, :, None, :].expand(B, 1, nq, HD),
                             nvis[:, :, None, :].expand(B, 1, nq, 1), dt)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. the decode body
# ---------------------------------------------------------------------------------------------------------------------------------------
# n = pos + 1 on both sides of the 64-key half-step and the 128-key score step, the 64-lane softmax stride and the PV stride (64 / 128 /
# 256 keys at HD 256 / 128 / 64); fewer keys than PV key groups (8 / 16 / 32)
POS = [0, 6, 7, 8, 15, 16, 31, 32, 62, 63, 64, 126, 127, 128, 254, 255, 256, 300]
SLOTS = [7, 2, 17, 0, 5, 13, 9, 1, 18, 10, 4, 15, 8, 3, 12, 16, 11, 14]             # a non-monotone permutation of 18 of 19 slots (6 stays out)
S, LMAX_D = 19, 320
# G = 2 (Gemma), G = 4 (Mistral), G = 1 and G = 3: the last two take the min(g0 + 1, G - 1) arm of the two-heads-per-sweep PV
SHAPES_D = [(4, 2, 256, 50.0), (8, 2, 128, 0.0), (2, 2, 64, 50.0), (6, 2, 64, 0.0)]
SHAPE_D_IDS = ["hd256-g2", "hd128-g4", "hd64-g1", "hd64-g3"]
WINDOWS_D = [0, 200]


def split_qkv(qkv, nq, nkv, HD):
    M = qkv.shape[0]
    return (qkv[:, : nq * HD].reshape(M, nq, HD), qkv[:, nq * HD: (nq + nkv) * HD].reshape(M, nkv, HD),
            qkv[:, (nq + nkv) * HD:].reshape(M, nkv, HD))


def rope_in_dtype(q, k, cos, sin):
    """q [M, nq, HD], k [M, nkv, HD], cos / sin [M, HD], all in the model dtype: O.apply_rope evaluated in that dtype on the CPU — each
    product and the sum round to the dtype, the kernels' documented roundings"""
    qr, kr = O.apply_rope(q[:, :, None, :], k[:, :, None, :], cos[:, None, :], sin[:, None, :])
    assert qr.dtype == q.dtype
    return qr[:, :, 0, :], kr[:, :, 0, :]


def decode_case(dt, nq, nkv, HD, rows, pos_of_row, seed=160, zero_q=False, one_hot=False):
    """inputs of one decode launch of `rows` packed rows: qkv with a padded row stride, each row's own rope row, random caches"""
    kvd, W = nkv * HD, (nq + 2 * nkv) * HD
    qkv = seeded((rows, W + 8), seed, dtype=dt)[:, :W]
    if zero_q:
        qkv[:, : nq * HD] = 0
    if one_hot:
        v = torch.zeros((rows, nkv, HD), dtype=dt)
        v[torch.arange(rows), :, torch.tensor(pos_of_row) % HD] = 1.0
        qkv[:, (nq + nkv) * HD:] = v.reshape(rows, kvd)
    cos, sin = O.rope_cos_sin(torch.tensor([[p] for p in pos_of_row]), HD, 10000.0, dt)
    return qkv, cos.reshape(rows, HD).contiguous(), sin.reshape(rows, HD).contiguous()


@pytest.fixture(scope="module")
def decode_caches():
    memo = {}

    def get(dt, nkv, HD):
        key = (dt, nkv, HD)
        if key not in memo:
            memo[key] = (seeded((S, LMAX_D, nkv, HD), 161, dtype=dt), seeded((S, LMAX_D, nkv, HD), 162, dtype=dt),
                         one_hot_v(LMAX_D, nkv, HD, dt, (S,)))
        return memo[key]
    return get


def visible_decode(pos, window, L):
    p = torch.tensor(pos)[:, None]
    kj = torch.arange(L)[None, :]
    vis = kj <= p
    if window:
        vis = vis & (kj >= p - window)
    return vis[:, None, :]                                                            # [rows, 1, L]


def launch_rows(hip, qkv, cs, sn, kc0, vc0, *, nq, nkv, HD, window, cap):
    M = len(POS)
    kc, vc = kc0.reshape(S, LMAX_D, -1).cuda(), vc0.reshape(S, LMAX_D, -1).cuda()
    out = torch.full((M, nq * HD), SENTINEL, dtype=qkv.dtype, device="cuda")
    tab = torch.tensor([SLOTS, POS], dtype=torch.int32).cuda()
    assert hip.attn_text_decode_rows_fits(nq=nq, nkv=nkv, HD=HD, Lmax=LMAX_D, window=window, pos_max=max(POS))
    hip.attn_text_decode_rows(qkv.cuda(), kc, vc, cs.cuda(), sn.cuda(), out, tab[0], tab[1], M=M, pos_max=max(POS), B=S, Lmax=LMAX_D, nq=nq,
                              nkv=nkv, HD=HD, window=window, scale=HD ** -0.5, softcap=cap)
    return out.cpu().view(M, 1, nq, HD), kc.cpu().view(S, LMAX_D, nkv, HD), vc.cpu().view(S, LMAX_D, nkv, HD)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("nq,nkv,HD,cap", SHAPES_D, ids=SHAPE_D_IDS)
def test_decode_rows_against_fp64(hip, decode_caches, dt, nq, nkv, HD, cap):
    """rope in the dtype, append at pos, t2t_ref over lo .. pos; the appended K rows equal the dtype-eager rope and the appended V rows the
    raw v bit for bit; no other cache row moves"""
    M = len(POS)
    kc0, vc0, _ = decode_caches(dt, nkv, HD)
    qkv, cs, sn = decode_case(dt, nq, nkv, HD, M, POS)
    q, k, v = split_qkv(qkv, nq, nkv, HD)
    qr, kr = rope_in_dtype(q, k, cs, sn)
    kref, vref = kc0.clone(), vc0.clone()
    kref[SLOTS, POS], vref[SLOTS, POS] = kr, v
    for window in WINDOWS_D:
        ref = t2t_ref(qr[:, None], kref[SLOTS], vref[SLOTS], visible_decode(POS, window, LMAX_D), HD ** -0.5, cap, dt)
        out, kc, vc = launch_rows(hip, qkv, cs, sn, kc0, vc0, nq=nq, nkv=nkv, HD=HD, window=window, cap=cap)
        assert torch.equal(bits(kc[SLOTS, POS]), bits(kr)), f"window {window}: appended K rows != rope in the dtype"
        assert torch.equal(bits(vc[SLOTS, POS]), bits(v)), f"window {window}: appended V rows != raw v"
        assert torch.equal(bits(kc), bits(kref)) and torch.equal(bits(vc), bits(vref)), f"window {window}: a cache row outside the append moved"
        check(f"decode_rows window {window}", out, ref, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("nq,nkv,HD,cap", SHAPES_D, ids=SHAPE_D_IDS)
def test_decode_rows_key_census(hip, decode_caches, dt, nq, nkv, HD, cap):
    """the q part of qkv zero (rope keeps it zero), v_new one-hot at pos % HD, the V cache one-hot at j % HD"""
    M = len(POS)
    kc0, _, v10 = decode_caches(dt, nkv, HD)
    qkv, cs, sn = decode_case(dt, nq, nkv, HD, M, POS, zero_q=True, one_hot=True)
    for window in WINDOWS_D:
        count, nvis = census_expect(visible_decode(POS, window, LMAX_D), HD)
        out, _, vc = launch_rows(hip, qkv, cs, sn, kc0, v10, nq=nq, nkv=nkv, HD=HD, window=window, cap=cap)
        assert torch.equal(bits(vc), bits(v10)), f"window {window}: the one-hot V cache changed"          # v_new is the row it replaces
        check_census(f"census decode_rows window {window}", out, count[:, :, None, :].expand(M, 1, nq, HD),
                     nvis[:, :, None, :].expand(M, 1, nq, 1), dt)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("nq,nkv,HD,cap", SHAPES_D, ids=SHAPE_D_IDS)
@pytest.mark.parametrize("dyn", [False, True], ids=["host-pos", "device-pos"])
def test_decode_masked_against_fp64(hip, decode_caches, dt, nq, nkv, HD, cap, dyn):
    """vidi_attn_text_decode: B = 2 at one position, holes in batch row 1's key mask, the masked form of the body"""
    kc0, vc0, _ = decode_caches(dt, nkv, HD)
    kc0, vc0 = kc0[:B], vc0[:B]
    km = torch.ones((B, LMAX_D), dtype=torch.uint8)
    km[1, 3:6] = 0
    km[1, 58:63] = 0                                        # right below the 64-key half-step, inside every window used here
    for pos in (63, 64, 128, 129):
        qkv, cs, sn = decode_case(dt, nq, nkv, HD, B, [pos, pos - 3], seed=163)      # per-row rope positions (right-padded batch)
        q, k, v = split_qkv(qkv, nq, nkv, HD)
        qr, kr = rope_in_dtype(q, k, cs, sn)
        kref, vref = kc0.clone(), vc0.clone()
        kref[:, pos], vref[:, pos] = kr, v
        for window in (0, 40, 200):
            vis = visible_decode([pos, pos], window, LMAX_D) & km[:, None, :].bool()
            ref = t2t_ref(qr[:, None], kref, vref, vis, HD ** -0.5, cap, dt)
            kc, vc = kc0.reshape(B, LMAX_D, -1).cuda(), vc0.reshape(B, LMAX_D, -1).cuda()
            out = torch.full((B, nq * HD), SENTINEL, dtype=dt, device="cuda")
            assert hip.attn_text_decode_fits(nq=nq, nkv=nkv, HD=HD, Lmax=LMAX_D, window=window, pos0=None if dyn else pos)
            pos_dev = torch.tensor([pos], dtype=torch.int32, device="cuda") if dyn else None
            hip.attn_text_decode(qkv.cuda(), kc, vc, km.cuda(), cs.cuda(), sn.cuda(), out, B=B, Lmax=LMAX_D, nq=nq, nkv=nkv, HD=HD, window=window,
                                 scale=HD ** -0.5, softcap=cap, pos0=(0 if dyn else pos), pos_dev=pos_dev)
            assert torch.equal(bits(kc.cpu().view(B, LMAX_D, nkv, HD)), bits(kref)), f"pos {pos} window {window}: K cache"
            assert torch.equal(bits(vc.cpu().view(B, LMAX_D, nkv, HD)), bits(vref)), f"pos {pos} window {window}: V cache"
            check(f"decode pos {pos} window {window}", out.cpu().view(B, 1, nq, HD), ref, dt)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. rope roundings, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("HD", [64, 128, 256])
def test_rope_equals_the_dtype_eager_rope_bitwise(hip, dt, HD):
    """vidi_rope at positions 0 .. 300: three IEEE roundings on both sides (two products, one sum)"""
    nq, nkv, rows = 4, 2, 301
    q, k = seeded((rows, nq, HD), 170, dtype=dt), seeded((rows, nkv, HD), 171, dtype=dt)
    cos, sin = O.rope_cos_sin(torch.arange(rows)[:, None], HD, 10000.0, dt)
    cos, sin = cos.reshape(rows, HD).contiguous(), sin.reshape(rows, HD).contiguous()
    qr, kr = rope_in_dtype(q, k, cos, sin)
    qd, kd = q.reshape(rows, nq * HD).cuda(), k.reshape(rows, nkv * HD).cuda()
    hip.rope(qd, kd, cos.cuda(), sin.cuda(), rows=rows, nq=nq, nkv=nkv, HD=HD)
    assert torch.equal(bits(qd.cpu()), bits(qr.reshape(rows, nq * HD)))
    assert torch.equal(bits(kd.cpu()), bits(kr.reshape(rows, nkv * HD)))


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("HD", [64, 128, 256])
@pytest.mark.parametrize("dyn", [False, True], ids=["host-pos", "device-pos"])
def test_rope_cache_equals_the_dtype_eager_rope_bitwise(hip, dt, HD, dyn):
    """vidi_rope_cache: q rows, the appended K rows and the copied V rows at positions 0 .. 6 and 294 .. 300"""
    nq, nkv, Lq, Lmax = 4, 2, 7, 304
    kvd, rows = nkv * HD, B * Lq
    for past in (0, 294):
        qkv = seeded((rows, (nq + 2 * nkv) * HD + 16), 172, dtype=dt)[:, : (nq + 2 * nkv) * HD]          # row stride != width
        cos, sin = O.rope_cos_sin(torch.arange(past, past + Lq)[None].repeat(B, 1), HD, 10000.0, dt)
        cos, sin = cos.reshape(rows, HD).contiguous(), sin.reshape(rows, HD).contiguous()
        q, k, v = split_qkv(qkv, nq, nkv, HD)
        qr, kr = rope_in_dtype(q, k, cos, sin)
        kc0, vc0 = seeded((B, Lmax, kvd), 173, dtype=dt), seeded((B, Lmax, kvd), 174, dtype=dt)
        kref, vref = kc0.clone(), vc0.clone()
        kref[:, past: past + Lq], vref[:, past: past + Lq] = kr.reshape(B, Lq, kvd), v.reshape(B, Lq, kvd)
        kc, vc = kc0.cuda(), vc0.cuda()
        out = torch.full((rows, nq * HD), SENTINEL, dtype=dt, device="cuda")
        pos_dev = torch.tensor([past], dtype=torch.int32, device="cuda") if dyn else None
        hip.rope_cache(qkv.cuda(), out, kc, vc, cos.cuda(), sin.cuda(), B=B, Lq=Lq, Lmax=Lmax, nq=nq, nkv=nkv, HD=HD,
                       pos0=(0 if dyn else past), pos_dev=pos_dev)
        assert torch.equal(bits(out.cpu()), bits(qr.reshape(rows, nq * HD))), f"past {past}: q"
        assert torch.equal(bits(kc.cpu()), bits(kref)), f"past {past}: K cache"
        assert torch.equal(bits(vc.cpu()), bits(vref)), f"past {past}: V cache"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. what the dispatcher refuses (it returns before any launch)
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("why,Lmax,nq,nkv,HD,past,Lq", [
    ("past_len + Lq > Lmax", 32, 4, 2, 64, 30, 3),
    ("HD = 96", 32, 4, 2, 96, 4, 3),
    ("nq % nkv != 0", 32, 5, 2, 64, 4, 3),
    ("(HD + past + Lq) * 4 bytes of LDS > 64 KB", 16384, 1, 1, 64, 16383, 1),
])
def test_attn_text_refuses(hip, why, Lmax, nq, nkv, HD, past, Lq):
    dt = torch.bfloat16
    q = torch.zeros((Lq, nq * HD), dtype=dt, device="cuda")
    kc = torch.zeros((1, Lmax, nkv * HD), dtype=dt, device="cuda")
    out = torch.full((Lq, nq * HD), SENTINEL, dtype=dt, device="cuda")
    with pytest.raises(hip.VidiHipError):
        hip.attn_text(q, kc, kc, None, out, B=1, Lq=Lq, Lmax=Lmax, nq=nq, nkv=nkv, HD=HD, past_len=past, window=0, scale=HD ** -0.5, softcap=0.0)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), f"{why}: the output buffer changed"
