"""In-flight batching on the GPU: vidi_attn_text_decode_rows against vidi_attn_text_decode on each slot (bit for bit) and against the fp32
formulation, the engine's text slots against the CPU oracle, and `generate_inflight()` against the same engine's per-prompt plain runs."""
import pytest
import torch

import vidi_oracle as O
from test_gpu_multivideo import new_model, timed
from test_gpu_spec_decode import video
from test_inflight import NEW, PROMPTS, InflightOracleEngine
from util import logit_tol, report, seeded

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(scope="module")
def hip():
    from vidi_amd import hip as h
    h.load_library()
    return h


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------------------------------------------
S, LMAX = 12, 320
SLOTS = [7, 2, 11, 0, 5, 9, 1, 10, 4, 8, 3]                         # a non-monotone permutation of 11 of the 12 slots (6 stays out)
# one key; both sides of the 128-key score step; both sides of the PV key-group stride (8 x 256 / (HD / 8) = 256 / 128 / 64 keys at HD 64 / 128 / 256)
POS = [0, 1, 63, 64, 127, 128, 129, 255, 256, 257, 300]
SENTINEL = 7.0


def bits(t):
    return t.view(torch.int16)


def case(dt, nq, nkv, HD, slots, pos):
    """inputs of one launch: qkv rows with a padded stride, rope rows of each row's own position, random caches"""
    M, kvd = len(slots), nkv * HD
    qkv = seeded((M, nq * HD + 2 * kvd + 8), 90, dtype=dt)[:, : nq * HD + 2 * kvd].cuda()
    cos, sin = O.rope_cos_sin(torch.tensor([[max(p, 0)] for p in pos]), HD, 10000.0, dt)
    cs, sn = cos.reshape(M, HD).contiguous().cuda(), sin.reshape(M, HD).contiguous().cuda()
    kc0, vc0 = seeded((S, LMAX, kvd), 91, dtype=dt).cuda(), seeded((S, LMAX, kvd), 92, dtype=dt).cuda()
    tab = torch.tensor([slots, pos], dtype=torch.int32).cuda()
    return qkv, cs, sn, kc0, vc0, tab


def one_by_one(hip, qkv, cs, sn, kc, vc, out, rows, slots, pos, **kw):
    """vidi_attn_text_decode with B = 1 on each listed row's slot view of the caches at pos0 = pos[m]"""
    for m in rows:
        s, p = slots[m], pos[m]
        hip.attn_text_decode(qkv[m: m + 1], kc[s: s + 1], vc[s: s + 1], None, cs[m: m + 1], sn[m: m + 1], out[m: m + 1], B=1, pos0=p, **kw)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("HD", [64, 128, 256])
@pytest.mark.parametrize("nq,nkv", [(4, 2), (8, 2)])
def test_rows_kernel_equals_the_one_row_kernel_on_every_slot(hip, dt, HD, nq, nkv):
    """same body, same summation order: outputs and appended K/V rows bit for bit, every other cache byte untouched"""
    M = len(SLOTS)
    qkv, cs, sn, kc0, vc0, tab = case(dt, nq, nkv, HD, SLOTS, POS)
    appended = torch.zeros((S, LMAX), dtype=torch.bool, device="cuda")
    appended[torch.tensor(SLOTS).cuda(), torch.tensor(POS).cuda()] = True
    for window in (0, 16, 200):
        for cap in (0.0, 50.0):
            kw = dict(Lmax=LMAX, nq=nq, nkv=nkv, HD=HD, window=window, scale=HD ** -0.5, softcap=cap)
            assert hip.attn_text_decode_rows_fits(nq=nq, nkv=nkv, HD=HD, Lmax=LMAX, window=window, pos_max=max(POS))
            kc_a, vc_a = kc0.clone(), vc0.clone()
            ref = torch.full((M, nq * HD), SENTINEL, dtype=dt, device="cuda")
            one_by_one(hip, qkv, cs, sn, kc_a, vc_a, ref, range(M), SLOTS, POS, **kw)
            kc_b, vc_b = kc0.clone(), vc0.clone()
            out = torch.full((M, nq * HD), SENTINEL, dtype=dt, device="cuda")
            hip.attn_text_decode_rows(qkv, kc_b, vc_b, cs, sn, out, tab[0], tab[1], M=M, pos_max=max(POS), B=S, **kw)
            name = f"window {window}, softcap {cap}"
            assert torch.isfinite(out.float()).all() and not bool((out == SENTINEL).all(dim=1).any()), name
            assert torch.equal(bits(out), bits(ref)), name
            assert torch.equal(bits(kc_b), bits(kc_a)) and torch.equal(bits(vc_b), bits(vc_a)), name
            for c, c0 in ((kc_b, kc0), (vc_b, vc0)):
                assert torch.equal(bits(c)[~appended], bits(c0)[~appended]), name        # nothing outside the M appended rows moved
                assert not torch.equal(bits(c)[appended], bits(c0)[appended]), name


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_rows_kernel_skips_idle_and_out_of_range_records(hip, dt):
    """slot -1 (idle row), a position beyond pos_max, a slot beyond the caches and a position beyond the cache: outputs and caches untouched"""
    nq, nkv, HD = 8, 2, 128
    slots = [3, -1, 5, 2, S, 9]
    pos = [10, 4, 40, 7, 3, LMAX]
    pos_max = 20
    live = [0, 3]
    M = len(slots)
    qkv, cs, sn, kc0, vc0, tab = case(dt, nq, nkv, HD, slots, pos)
    kw = dict(Lmax=LMAX, nq=nq, nkv=nkv, HD=HD, window=0, scale=HD ** -0.5, softcap=50.0)
    kc_a, vc_a = kc0.clone(), vc0.clone()
    ref = torch.full((M, nq * HD), SENTINEL, dtype=dt, device="cuda")
    one_by_one(hip, qkv, cs, sn, kc_a, vc_a, ref, live, slots, pos, **kw)
    kc_b, vc_b = kc0.clone(), vc0.clone()
    out = torch.full((M, nq * HD), SENTINEL, dtype=dt, device="cuda")
    hip.attn_text_decode_rows(qkv, kc_b, vc_b, cs, sn, out, tab[0], tab[1], M=M, pos_max=pos_max, B=S, **kw)
    assert torch.equal(bits(out), bits(ref))
    assert bool((out[[1, 2, 4, 5]] == SENTINEL).all()) and not bool((out[live] == SENTINEL).all(dim=1).any())
    assert torch.equal(bits(kc_b), bits(kc_a)) and torch.equal(bits(vc_b), bits(vc_a))
    # a table of skipped records only leaves everything as it was
    kc_c, vc_c = kc0.clone(), vc0.clone()
    out.fill_(SENTINEL)
    idle = torch.tensor([[-1, 5], [0, 40]], dtype=torch.int32).cuda()
    hip.attn_text_decode_rows(qkv, kc_c, vc_c, cs, sn, out, idle[0], idle[1], M=2, pos_max=pos_max, B=S, **kw)
    assert bool((out == SENTINEL).all()) and torch.equal(bits(kc_c), bits(kc0)) and torch.equal(bits(vc_c), bits(vc0))


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_rows_kernel_against_the_fp32_formulation(hip, dt):
    """second anchor (the bitwise test would pass if both kernels shared a mistake): rope, append, windowed softmax and PV in plain fp32
    torch on the same inputs.  Bound: util.logit_tol's rule — 5 % (bf16) / 1 % (fp16) of the reference's spread, absolute."""
    nq, nkv, HD, window, cap = 8, 2, 128, 16, 50.0
    G, half, M = nq // nkv, HD // 2, len(SLOTS)
    qkv, cs, sn, kc0, vc0, tab = case(dt, nq, nkv, HD, SLOTS, POS)
    kc, vc = kc0.clone(), vc0.clone()
    out = torch.full((M, nq * HD), SENTINEL, dtype=dt, device="cuda")
    hip.attn_text_decode_rows(qkv, kc, vc, cs, sn, out, tab[0], tab[1], M=M, pos_max=max(POS), B=S, Lmax=LMAX, nq=nq, nkv=nkv, HD=HD,
                              window=window, scale=HD ** -0.5, softcap=cap)
    f = lambda t: t.float().cpu()                                                       # noqa: E731
    q = f(qkv)[:, : nq * HD].view(M, nq, HD)
    k = f(qkv)[:, nq * HD: nq * HD + nkv * HD].view(M, nkv, HD)
    v = f(qkv)[:, nq * HD + nkv * HD:].view(M, nkv, HD)
    c, s_ = f(cs)[:, None, :], f(sn)[:, None, :]
    rot = lambda x: torch.cat((-x[..., half:], x[..., :half]), dim=-1)                 # noqa: E731
    qr, kr = q * c + rot(q) * s_, k * c + rot(k) * s_
    kref, vref = f(kc0).view(S, LMAX, nkv, HD).clone(), f(vc0).view(S, LMAX, nkv, HD).clone()
    ref = torch.zeros((M, nq, HD))
    for m, (sl, p) in enumerate(zip(SLOTS, POS)):
        kref[sl, p], vref[sl, p] = kr[m].to(dt).float(), v[m]
        lo = max(0, p - window)
        for h in range(nq):
            kk, vv = kref[sl, lo: p + 1, h // G], vref[sl, lo: p + 1, h // G]
            sc = (kk @ qr[m, h]) * HD ** -0.5
            sc = cap * torch.tanh(sc / cap)
            ref[m, h] = torch.softmax(sc, dim=0) @ vv
    ref = ref.view(M, nq * HD)
    report("rows kernel vs fp32 torch", out, ref, logit_tol(dt, ref), 0.0)
    report("appended keys vs fp32 rope", kc.view(S, LMAX, nkv, HD)[torch.tensor(SLOTS).cuda(), torch.tensor(POS).cuda()], kr, logit_tol(dt, kr), 0.0)
    assert torch.equal(f(vc).view(S, LMAX, nkv, HD)[torch.tensor(SLOTS), torch.tensor(POS)], v)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. the engine's text slots against the CPU oracle
# ---------------------------------------------------------------------------------------------------------------------------------------
ADMIT = [[2, 21, 22], list(range(40, 49)), list(range(130, 151)), list(range(60, 72))]          # 3, 9, 21, 12 tokens: tiny's window (16) ends inside one
REFILL = [list(range(80, 95)), [2, 30, 31, 32, 33]]
FEED = [[201, 202, 203, 204], [211, 212, 213, 214, 215], [221, 222, 223, 224]]


def slot_steps(eng, mm):
    """4 ragged prompts admitted together, a step on all four, one slot retired and two admitted (the freed slot and a fresh one), a step on five
    rows, another slot retired, a last step -> the logits of every call (the fed tokens are given: every engine sees the same inputs)"""
    lg = lambda h: eng.logits_argmax(h)[0].float().cpu().clone()                        # noqa: E731
    ts = eng.new_text_slots(6, 40)
    outs = [lg(eng.slots_prefill(ts, [2, 0, 3, 1], ADMIT, mm))]
    outs.append(lg(eng.slots_decode(ts, [0, 1, 2, 3], FEED[0], mm)))
    ts.length[0] = -1
    outs.append(lg(eng.slots_prefill(ts, [0, 4], REFILL, mm)))
    assert ts.length[:5] == [15, 13, 4, 22, 5]
    outs.append(lg(eng.slots_decode(ts, [0, 1, 2, 3, 4], FEED[1], mm)))
    ts.length[3] = -1
    outs.append(lg(eng.slots_decode(ts, [0, 1, 2, 4], FEED[2], mm)))
    assert ts.length == [17, 15, 6, -1, 7, -1]
    return outs


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("arch", ["tiny", "tiny_7b"])
def test_engine_slots_against_the_oracle(arch, dt):
    from vidi_amd import config
    from vidi_amd.model import VidiForCausalLM
    cfg = getattr(config, arch)()
    model, w32 = new_model(cfg, dt, seed=3)
    om = VidiForCausalLM(cfg, w32, dtype=torch.float32, device="cpu", engine=InflightOracleEngine(cfg, w32))
    refs = slot_steps(om.engine, om.encode_mm_state(*video(cfg, torch.float32, "cpu")))
    eng = model.engine
    assert eng.max_inflight_rows() == 32 // (cfg.num_attention_heads // cfg.num_key_value_heads)
    mm = model.encode_mm_state(*video(cfg, dt, "cuda"))
    got, names = timed(lambda: slot_steps(eng, mm))
    for name, g, r in zip(("admit 4", "step on 4 rows", "retire 1, admit 2", "step on 5 rows", "retire 1, step on 4 rows"), got, refs):
        report(name, g, r, logit_tol(dt, r), 0.0)
    assert names.count("vidi_attn_text_decode_rows") == 3 * cfg.num_hidden_layers       # one per layer per decode step
    assert "vidi_attn_text_decode" not in names and "vidi_attn_text_decode_merge2" not in names
    assert "vidi_attn_text" in names and "vidi_rope_cache" in names                    # the ragged prefills


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. generate_inflight() against the per-prompt plain generate() of the same engine
# ---------------------------------------------------------------------------------------------------------------------------------------
# (config overrides, weight seed): chosen on the CPU oracle with tests/test_inflight.py's prompts, lengths and video — for weight seeds 1..12 the
# plain run of every prompt was decoded in fp32 and the positions in front of its first step with a top-2 margin <= 2 x logit_tol(bf16) counted;
# the seed with the most compared positions whose answers also differ between prompts was taken: 44 of 44 (Vidi1.5, untied head: tied random
# embeddings echo their input) and 38 of 44 (Vidi-7B) on the oracle.
GEN_CASES = {"vidi15": (dict(tie_word_embeddings=False), 7), "vidi7b": ({}, 7)}


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("arch", ["vidi15", "vidi7b"])
def test_generate_inflight_against_plain_greedy(arch, dt):
    from vidi_amd import config
    over, seed = GEN_CASES[arch]
    cfg = (config.tiny if arch == "vidi15" else config.tiny_7b)(**over)
    model, _ = new_model(cfg, dt, seed=seed)
    mm = model.encode_mm_state(*video(cfg, dt, "cuda"))
    plain, n_cmp = [], []
    for p, n in zip(PROMPTS, NEW):
        full = model.generate(torch.tensor([p]), mm_state=mm, max_new_tokens=n, eos_token_id=999999, return_dict_in_generate=True, output_logits=True)
        logits = torch.cat([l.float().cpu() for l in full.logits])
        ltol = logit_tol(dt, logits)
        margin = [float(torch.topk(l, 2).values.diff().abs()) for l in logits]
        plain.append(full.sequences[0].tolist())
        n_cmp.append(next((t for t, m in enumerate(margin) if m <= 2 * ltol), n))       # compared up to the first low-margin step of the plain run
        assert len(plain[-1]) == n
    print(f"{arch}: compared positions per prompt {n_cmp} of {NEW}")
    assert 2 * sum(n_cmp) >= sum(NEW), "fewer than half of the positions are compared: pick other seeds"
    seen = []
    got, names = timed(lambda: model.generate_inflight([torch.tensor(p) for p in PROMPTS], mm_state=mm, max_new_tokens=NEW, eos_token_id=999999,
                                                       max_rows=3, on_finish=lambda i, t: seen.append(i)))
    assert sorted(seen) == list(range(len(PROMPTS)))
    for i, (g, p, k) in enumerate(zip(got, plain, n_cmp)):
        assert g.device.type == "cuda" and len(g) == NEW[i]
        assert g.tolist()[:k] == p[:k], (i, g.tolist(), p, k)
    assert "vidi_attn_text_decode_rows" in names and "vidi_attn_text_decode" not in names


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. what text_forward(rows=...) refuses
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_rows_refusals():
    from vidi_amd.config import tiny
    from vidi_amd.engine import MMBatchState
    cfg = tiny()
    model, _ = new_model(cfg, torch.bfloat16, seed=3)
    eng = model.engine
    ts = eng.new_text_slots(2, 24)
    eng.slots_prefill(ts, [1], [[2, 21, 22]], None)
    tab = torch.tensor([[1], [3]], dtype=torch.int32).cuda()
    emb = eng.embed_tokens(torch.tensor([30]).cuda())
    posn = torch.tensor([3]).cuda()
    rows = (ts, tab[0], tab[1], 3)
    assert eng.text_forward(emb, posn, None, None, Lq=1, rows=rows).shape == (1, cfg.hidden_size)       # the supported call
    with pytest.raises(RuntimeError, match="dyn"):
        eng.text_forward(emb, posn, None, None, Lq=1, dyn=True, rows=rows)
    with pytest.raises(RuntimeError, match="MMBatchState"):
        eng.text_forward(emb, posn, None, MMBatchState.__new__(MMBatchState), Lq=1, rows=rows)
    with pytest.raises(RuntimeError):
        eng.slots_decode(ts, [1], [30], MMBatchState.__new__(MMBatchState))
    eng.sharded = True
    try:
        with pytest.raises(RuntimeError, match="sharded"):
            eng.text_forward(emb, posn, None, None, Lq=1, rows=rows)
    finally:
        eng.sharded = False
    # a slot so long that the scores of a full-attention layer do not fit the kernel's 64 KB of LDS: no fallback
    big = eng.new_text_slots(1, 9000)
    big.length[0] = 8500
    from vidi_amd import hip as h
    assert not h.attn_text_decode_rows_fits(nq=cfg.num_attention_heads, nkv=cfg.num_key_value_heads, HD=cfg.head_dim, Lmax=9000, window=0, pos_max=8500)
    with pytest.raises(RuntimeError, match="does not fit"):
        eng.slots_decode(big, [0], [30], None)
    assert big.length[0] == 8500
    with pytest.raises(ValueError):
        eng.slots_decode(ts, [0], [30], None)                                            # a free slot
    with pytest.raises(ValueError):
        eng.slots_prefill(ts, [1], [[2, 3]], None)                                       # a slot in use
