"""Per-token log-probabilities on the GPU: vidi_token_logprob against fp64 on the CPU, `VidiEngine.token_logprobs` against `logits_argmax`'s
logits, `score()` against the CPU oracle and `generate_inflight(output_logprobs=True)` against the same call with the flag off.

Bound on lse / logprob: 5e-5 absolute against fp64 from the same rounded values, |x| <= 64.  Summation chains are under 100 long after the
per-thread / tree split (<= 100 x 2^-24 = 6e-6 relative on the sum = absolute on its log), a few ulp from exp on the terms that matter, one
fp32 rounding each of lse and x_t - lse at magnitude <= 64 (2 x 3.8e-6): about 1.5e-5 at worst, times three."""
import numpy as np
import pytest
import torch

from test_gpu_inflight import GEN_CASES
from test_gpu_multivideo import new_model, timed
from test_gpu_spec_decode import video
from test_inflight import NEW, PROMPTS
from test_score import PROMPT, ScoreOracleEngine
from util import logit_tol

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
BOUND = 5e-5


@pytest.fixture(scope="module")
def hip():
    from vidi_amd import hip as h
    h.load_library()
    return h


def rand_logits(shape, seed, dt):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 60.0 - 30.0).to(dt)


def ref64(x, targets=None):
    """fp64 on the CPU from the values x [R, V] (already rounded to the model dtype): -> (first argmax, lse, logprob, rank) by the definition"""
    x = x.detach().cpu().double()
    R, V = x.shape
    idx = torch.from_numpy(np.argmax(x.numpy(), axis=1))                                # numpy: the first of equal maxima
    t = torch.full((R,), -1, dtype=torch.int64) if targets is None else targets.detach().cpu().clone()
    t = torch.where(t == -1, idx, t)
    ok = (t >= 0) & (t < V)
    tc = t.clamp(0, V - 1)
    xt = x.gather(1, tc[:, None])
    lse = torch.logsumexp(x, dim=-1)
    lp = torch.where(ok, xt[:, 0] - lse, torch.full_like(lse, -float("inf")))
    rank = ((x > xt) | ((x == xt) & (torch.arange(V)[None] < tc[:, None]))).sum(-1)
    return idx, lse, lp, torch.where(ok, rank, torch.full_like(rank, -1))


def check(name, got, ref):
    idx, lse, lp, rank = (t.cpu() for t in got)
    ridx, rlse, rlp, rrank = ref
    fin = torch.isfinite(rlp)
    e_lse = float((lse.double() - rlse).abs().max())
    e_lp = float((lp.double()[fin] - rlp[fin]).abs().max()) if bool(fin.any()) else 0.0
    print(f"{name}: max |lse - fp64| = {e_lse:.3g}, max |logprob - fp64| = {e_lp:.3g} (bound {BOUND})")
    assert torch.equal(idx, ridx), name
    assert torch.equal(rank.long(), rrank), name
    assert torch.equal(lp[~fin], rlp[~fin].float()), name                                # -inf where the reference has it
    assert e_lse <= BOUND and e_lp <= BOUND, (name, e_lse, e_lp)
    return max(e_lse, e_lp)


def targets_for(R, V, seed):
    """a mix of given tokens and -1 (the greedy one)"""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, V, (R,), generator=g)
    t[::3] = -1
    return t


# (V, R): scalar path with fewer entries than threads; 125 vectors, fewer than a block's threads (1000 IS a multiple of 8, so these rows take the
# 16-byte loads); 1001: the scalar path over four blocks; exactly one block of vectors; one vector into the second block; one vector past 128
# full blocks (the grid-stride loop's second trip); the model's vocabulary
SHAPES = [(7, 3), (1000, 3), (1001, 3), (2048, 3), (2056, 3), (262152, 3), (256000, 2)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("V,R", SHAPES)
def test_kernel_without_softcap_against_fp64(hip, dt, V, R):
    """cap = 0: every output against fp64 from the raw logits, a fully independent reference; with targets, with -1 and without a table"""
    x = rand_logits((R, V), 100 + V % 97, dt)
    xd = x.cuda()
    t = targets_for(R, V, V)
    check(f"V={V} targets", hip.token_logprob(xd, t.cuda(), 0.0), ref64(x, t))
    got = hip.token_logprob(xd, None, 0.0)
    ref = ref64(x, None)
    check(f"V={V} no table", got, ref)
    assert got[3].tolist() == [0] * R and torch.equal(got[2].cpu(), (x.float().max(-1).values - got[1].cpu()))      # rank 0, logprob = max - lse
    minus1 = hip.token_logprob(xd, torch.full((R,), -1, dtype=torch.int64).cuda(), 0.0)
    assert all(torch.equal(a, b) for a, b in zip(got, minus1))
    assert torch.equal(xd.cpu().view(torch.int16), x.view(torch.int16))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("V,R", SHAPES)
def test_kernel_with_softcap_against_the_argmax_kernel(hip, dt, V, R):
    """cap = 30: vidi_softcap_argmax on a clone leaves the rounded x_i in place — same idx, and lse / logprob / rank against fp64 from those values"""
    x = rand_logits((R, V), 200 + V % 97, dt)
    xd = x.cuda()
    clone = xd.clone()
    idx2 = torch.empty((R,), dtype=torch.int64, device="cuda")
    hip.softcap_argmax(clone, idx2, 30.0)
    t = targets_for(R, V, V + 1)
    got = hip.token_logprob(xd, t.cuda(), 30.0)
    assert torch.equal(got[0], idx2)
    assert not torch.equal(clone.view(torch.int16), xd.view(torch.int16))                # the clone was capped in place ...
    assert torch.equal(xd.cpu().view(torch.int16), x.view(torch.int16))                  # ... the source is bitwise unchanged
    check(f"V={V} cap 30", got, ref64(clone, t))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("V", [2048, 2056])
def test_kernel_strided_and_unaligned_rows(hip, dt, V):
    R = 3
    x = rand_logits((R, V), 300 + V, dt)
    t = targets_for(R, V, 5)
    ref = ref64(x, t)
    for name, ld, off in (("ld = V + 8", V + 8, 0), ("ld = V + 3: scalar path", V + 3, 0), ("base off by one element", V + 8, 1)):
        buf = torch.full((R * ld + off,), 99.0, dtype=dt, device="cuda")                 # 99 between the rows: read by mistake, it would be the maximum
        view = buf[off:].view(R, ld)[:, :V]
        view.copy_(x)
        assert view.stride(0) == ld and (view.data_ptr() % 16 == 0) == (off == 0)
        check(f"V={V} {name}", hip.token_logprob(view, t.cuda(), 0.0), ref)
        check(f"V={V} {name}, cap 30", hip.token_logprob(view, t.cuda(), 30.0), ref64(capped(hip, x), t))


def capped(hip, x):
    c = x.cuda().clone()
    hip.softcap_argmax(c, torch.empty((x.shape[0],), dtype=torch.int64, device="cuda"), 30.0)
    return c


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_kernel_row_count_beyond_the_grid_limit(hip, dt):
    R, V = 70000, 16
    x = rand_logits((R, V), 7, dt)
    t = targets_for(R, V, 8)
    check("R=70000", hip.token_logprob(x.cuda(), t.cuda(), 0.0), ref64(x, t))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("V", [1001, 2056])
def test_kernel_ties(hip, dt, V):
    R = 3
    x = rand_logits((R, V), 400 + V, dt)
    x[0, 700], x[0, 41] = 31.0, 31.0                                 # the maximum twice: the first index wins
    v = x[1, 500].clone()
    x[1, 100], x[1, 900] = v, v                                      # the target's value once in front of it and once behind
    t = torch.tensor([-1, 500, 41])
    for cap in (0.0, 30.0):
        vals = x if cap == 0.0 else capped(hip, x).cpu()
        got = hip.token_logprob(x.cuda(), t.cuda(), cap)
        check(f"ties V={V} cap {cap}", got, ref64(vals, t))
        assert int(got[0][0]) == 41 and int(got[3][0]) == 0
        above = int((vals[1].double() > float(vals[1, 500])).sum())
        same_in_front = int((vals[1, :500].double() == float(vals[1, 500])).sum())
        assert same_in_front >= 1 and int(got[3][1]) == above + same_in_front
    # the tied maximum given as a target: the second of the two has rank 1
    got = hip.token_logprob(x.cuda(), torch.tensor([700, -1, -1]).cuda(), 0.0)
    assert int(got[3][0]) == 1 and int(got[0][0]) == 41


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_kernel_targets_out_of_range_are_skipped(hip, dt):
    R, V, GUARD = 4, 2056, 64
    x = rand_logits((R, V), 55, dt)
    buf = torch.full((R * V + GUARD,), 77.0, dtype=dt, device="cuda")       # the guard behind the logits: index V of the last row is its first entry
    view = buf[: R * V].view(R, V)
    view.copy_(x)
    t = torch.tensor([V, -2, 5, V + 100000])
    got = hip.token_logprob(view, t.cuda(), 0.0)
    check("out of range", got, ref64(x, t))
    assert got[2].tolist()[0] == -float("inf") and got[2].tolist()[1] == -float("inf") and got[3].tolist() == [-1, -1, int(got[3][2]), -1]
    assert bool((buf[R * V:] == 77.0).all()) and torch.equal(view.cpu().view(torch.int16), x.view(torch.int16))
    with pytest.raises(hip.VidiHipError, match="bad shape"):                 # a workspace for fewer rows than the call has
        hip.token_logprob(view, None, 0.0, workspace=hip.token_logprob_workspace(R - 1, "cuda"))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("V", [1000, 1001, 2056, 262152])
def test_kernel_is_deterministic_and_rows_are_independent(hip, dt, V):
    R = 3
    xd = rand_logits((R, V), 500 + V % 89, dt).cuda()
    t = targets_for(R, V, 9).cuda()
    bits = lambda o: [o[0], o[1].view(torch.int32), o[2].view(torch.int32), o[3]]      # noqa: E731
    a, b = hip.token_logprob(xd, t, 30.0), hip.token_logprob(xd, t, 30.0)
    assert all(torch.equal(p, q) for p, q in zip(bits(a), bits(b)))
    for r in range(R):
        alone = hip.token_logprob(xd[r: r + 1], t[r: r + 1], 30.0)
        assert all(torch.equal(p[r: r + 1], q) for p, q in zip(bits(a), bits(alone))), r


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. the engine
# ---------------------------------------------------------------------------------------------------------------------------------------
def hidden_rows(model, n=11):
    """the final hidden rows of an n-token text prompt"""
    eng = model.engine
    ids = torch.arange(20, 20 + n, dtype=torch.int64, device="cuda")
    ts = eng.new_text_state(1, n + 1)
    return eng.text_forward(eng.embed_tokens(ids), torch.arange(n, device="cuda"), ts, None, Lq=n).clone()


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("arch", ["tiny", "tiny_7b"])
def test_engine_token_logprobs_against_logits_argmax(arch, dt):
    from vidi_amd import config
    cfg = getattr(config, arch)()
    model, _ = new_model(cfg, dt, seed=3)
    eng = model.engine
    hn = hidden_rows(model)
    logits, ids = eng.logits_argmax(hn)                               # the same M: the same projection kernel, the same bits
    (got_ids, lp, rank), names = timed(lambda: eng.token_logprobs(hn))
    assert names.count("vidi_token_logprob") == 1 and "vidi_softcap_argmax" not in names
    assert got_ids.dtype == torch.int64 and lp.dtype == torch.float32 and rank.dtype == torch.int32
    assert torch.equal(got_ids, ids) and rank.tolist() == [0] * hn.shape[0]
    _, _, rlp, _ = ref64(logits)
    err = float((lp.cpu().double() - rlp).abs().max())
    print(f"{arch}: greedy logprob vs fp64 from logits_argmax's logits: {err:.3g}")
    assert err <= BOUND
    # chunking: lm_head on at most chunk_rows rows at a time
    g = torch.Generator().manual_seed(3)
    t = torch.randint(0, cfg.vocab_size, (hn.shape[0],), generator=g)
    _, _, rlp_t, rrank_t = ref64(logits, t)
    for chunk in (1, 5, 256):
        (cid, clp, crank), names = timed(lambda: eng.token_logprobs(hn, t.cuda(), chunk_rows=chunk))
        assert names.count("vidi_token_logprob") == -(-hn.shape[0] // chunk)
        err = float((clp.cpu().double() - rlp_t).abs().max())
        print(f"{arch}: chunk_rows = {chunk}: logprob vs fp64: {err:.3g}; ranks equal: {torch.equal(crank.cpu().long(), rrank_t)}")
        assert torch.equal(cid, ids), chunk
        assert err <= BOUND, chunk


class RecordingOracle(ScoreOracleEngine):
    def token_logprobs(self, hn, targets=None, chunk_rows=256):
        self.logits = super(ScoreOracleEngine, self).logits_argmax(hn)[0].float()
        return super().token_logprobs(hn, targets, chunk_rows)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("arch", ["tiny", "tiny_7b"])
def test_score_against_the_oracle(arch, dt):
    """each logit is within logit_tol of the oracle's by the project's contract, so x_t and lse each move by at most that: 2 x logit_tol a token"""
    from vidi_amd import config
    from vidi_amd.model import VidiForCausalLM
    cfg = getattr(config, arch)()
    model, w32 = new_model(cfg, dt, seed=3)
    oeng = RecordingOracle(cfg, w32)
    om = VidiForCausalLM(cfg, w32, dtype=torch.float32, device="cpu", engine=oeng)
    g = torch.Generator().manual_seed(17)
    cands = [torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist() for n in (1, 3, 6)]
    ref = om.score(PROMPT, cands, mm_state=om.encode_mm_state(*video(cfg, torch.float32, "cpu")))
    tol = 2 * logit_tol(dt, oeng.logits)
    mm = model.encode_mm_state(*video(cfg, dt, "cuda"))
    got, names = timed(lambda: model.score(PROMPT, cands, mm_state=mm))
    assert names.count("vidi_token_logprob") == 1 and "vidi_softcap_argmax" not in names       # the kernel, never the torch path
    for c, a, b in zip(cands, got, ref):
        err = float((a.token_logprobs.cpu() - b.token_logprobs).abs().max())
        print(f"{arch}: Lc = {len(c)}: max |logprob - oracle| = {err:.3g} (bound {tol:.3g}); ranks {a.ranks.tolist()} vs {b.ranks.tolist()}")
        assert a.token_logprobs.is_cuda and a.token_logprobs.shape == (len(c),) and a.ranks.dtype == torch.int32
        assert err <= tol
        assert a.logprob == pytest.approx(float(a.token_logprobs.double().sum()), abs=1e-6)
    one = model.score(PROMPT, cands, mm_state=mm, max_positions=1)   # one candidate per prefill: the same positions through other row counts
    for a, b in zip(one, ref):
        assert float((a.token_logprobs.cpu() - b.token_logprobs).abs().max()) <= tol


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. the in-flight loop
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("arch", ["vidi15", "vidi7b"])
def test_generate_inflight_output_logprobs_keeps_the_tokens(arch, dt):
    from vidi_amd import config
    over, seed = GEN_CASES[arch]
    cfg = (config.tiny if arch == "vidi15" else config.tiny_7b)(**over)
    model, _ = new_model(cfg, dt, seed=seed)
    mm = model.encode_mm_state(*video(cfg, dt, "cuda"))
    run = lambda **kw: model.generate_inflight([torch.tensor(p) for p in PROMPTS], mm_state=mm, max_new_tokens=NEW, eos_token_id=999999,      # noqa: E731
                                               max_rows=3, **kw)
    off = run()
    (toks, lps), names = timed(lambda: run(output_logprobs=True))
    assert [t.tolist() for t in toks] == [t.tolist() for t in off]
    assert "vidi_token_logprob" in names and "vidi_softcap_argmax" not in names
    for t, v in zip(toks, lps):
        assert v.dtype == torch.float32 and v.is_cuda and v.shape == t.shape
        assert bool(torch.isfinite(v).all()) and bool((v <= 0).all())
