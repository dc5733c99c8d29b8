"""Scoring candidate answers on the CPU: `VidiForCausalLM.score()` and `generate_inflight(output_logprobs=True)` over the CPU oracle engine,
`run_inflight(logprobs=True)` over the scripted engine of tests/test_inflight.py, and vidi_token_logprob's argument checks (no launch)."""
import ctypes
import os
import sys
from types import SimpleNamespace

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
sys.path.insert(0, HERE)

from oracle_engine import OracleEngine  # noqa: E402
from test_inflight import FakeEngine, InflightOracleEngine, expected, make_prompts, token  # noqa: E402
from util import seeded  # noqa: E402
from vidi_amd.inflight import run_inflight  # noqa: E402

PER_TOKEN = 1e-4                                                     # the oracle runs in fp32; only the batch composition differs between the paths compared


def torch_logprobs(logits, targets=None):
    """the definition in torch: (first argmax, log-softmax at the target (-1: the argmax), entries ranked in front of it) of fp32 rows"""
    x = logits.float()
    idx = torch.argmax(x, dim=-1)
    t = idx if targets is None else torch.where(targets < 0, idx, targets.to(idx.device))
    xt = x.gather(1, t[:, None])
    lp = (xt - torch.logsumexp(x, dim=-1, keepdim=True))[:, 0]
    col = torch.arange(x.shape[1])[None]
    rank = ((x > xt) | ((x == xt) & (col < t[:, None]))).sum(-1).to(torch.int32)
    return idx, lp, rank


class ScoreOracleEngine(InflightOracleEngine):
    """the oracle engine + `token_logprobs` (what VidiEngine computes with vidi_token_logprob), counting the prefill calls and the rows that
    reach lm_head"""

    def __init__(self, cfg, w):
        super().__init__(cfg, w)
        self.forwards, self.head_rows = [], 0

    def text_forward(self, hidden, positions, ts, mm, Lq, new_mask=None, dyn=False):
        self.forwards.append((ts.B, Lq))
        return super().text_forward(hidden, positions, ts, mm, Lq, new_mask=new_mask, dyn=dyn)

    def token_logprobs(self, hn, targets=None, chunk_rows=256):
        self.head_rows += hn.shape[0]
        return torch_logprobs(OracleEngine.logits_argmax(self, hn)[0], targets)


PROMPT = [2, 30, -200, 31, 32, 33]                                   # 5 text positions and the <image> placeholder
SEEDS = {"vidi15": 4, "vidi7b": 2}                                   # tests/test_inflight.py's
_cache = {}


def setup(arch):
    if arch not in _cache:
        from vidi_amd.config import tiny, tiny_7b
        from vidi_amd.model import VidiForCausalLM
        from vidi_amd.weights import init_random_weights
        cfg = tiny(tie_word_embeddings=False) if arch == "vidi15" else tiny_7b()
        w = init_random_weights(cfg, seed=SEEDS[arch], dtype=torch.float32, device="cpu")
        eng = ScoreOracleEngine(cfg, w)
        model = VidiForCausalLM(cfg, w, dtype=torch.float32, device="cpu", engine=eng)
        plain = VidiForCausalLM(cfg, w, dtype=torch.float32, device="cpu", engine=OracleEngine(cfg, w))      # no `token_logprobs`: score()'s torch path
        S = cfg.vis_image_size
        mm = model.encode_mm_state(seeded((2, 3, S, S), 702, 0.5).clamp(-1, 1)[None], seeded((1, cfg.aud_num_mel_bins, cfg.aud_nb_max_frames), 710, 0.3)[None], [100])
        g = torch.Generator().manual_seed(17)
        cands = [torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist() for n in (1, 3, 6)]
        _cache[arch] = SimpleNamespace(cfg=cfg, eng=eng, model=model, plain=plain, mm=mm, cands=cands)
    s = _cache[arch]
    s.eng.forwards, s.eng.head_rows = [], 0
    return s


@pytest.mark.parametrize("arch", ["vidi15", "vidi7b"])
def test_score_equals_the_loss_of_forward_with_labels(arch):
    """labels masked to the candidate: forward()'s mean cross-entropy x Lc is minus the candidate's summed log-probability"""
    s = setup(arch)
    got = s.model.score(PROMPT, s.cands, mm_state=s.mm)
    torch_path = s.plain.score(torch.tensor(PROMPT), [torch.tensor(c) for c in s.cands], mm_state=s.mm)
    assert s.eng.forwards == [(3, 5 + 6)] and s.eng.head_rows == 1 + 3 + 6        # one ragged prefill; lm_head on the candidate positions only
    for c, rec, rec2 in zip(s.cands, got, torch_path):
        n = len(c)
        ids = torch.tensor([PROMPT + c])
        labels = torch.tensor([[-100] * len(PROMPT) + c])
        loss = float(s.model.forward(ids, mm_state=s.mm, labels=labels).loss)
        print(f"{arch}: Lc = {n}: score {rec.logprob:.6f}, -loss x Lc {-loss * n:.6f}")
        assert rec.token_logprobs.shape == (n,) and rec.token_logprobs.dtype == torch.float32
        assert rec.ranks.shape == (n,) and rec.ranks.dtype == torch.int32 and bool((rec.ranks >= 0).all())
        assert bool((rec.token_logprobs < 0).all()) and rec.logprob == pytest.approx(float(rec.token_logprobs.double().sum()), abs=1e-6)
        assert rec.mean_logprob == pytest.approx(rec.logprob / n)
        assert abs(rec.logprob + loss * n) <= PER_TOKEN * n
        assert float((rec.token_logprobs - rec2.token_logprobs).abs().max()) <= PER_TOKEN and torch.equal(rec.ranks, rec2.ranks)


def test_packing_does_not_change_the_values():
    s = setup("vidi15")
    whole = s.model.score(PROMPT, s.cands, mm_state=s.mm, max_positions=512)
    calls = list(s.eng.forwards)
    s.eng.forwards = []
    single = s.model.score(PROMPT, s.cands, mm_state=s.mm, max_positions=1)
    assert calls == [(3, 11)] and s.eng.forwards == [(1, 6), (1, 8), (1, 11)]          # always at least one candidate per call
    s.eng.forwards = []
    s.model.score(PROMPT, s.cands, mm_state=s.mm, max_positions=2 * 8)                # rows x padded length <= 16: (1, 3 tokens) together, 6 alone
    assert s.eng.forwards == [(2, 8), (1, 11)]
    for a, b in zip(whole, single):
        assert float((a.token_logprobs - b.token_logprobs).abs().max()) <= PER_TOKEN
        assert torch.equal(a.ranks, b.ranks)


@pytest.mark.parametrize("arch", ["vidi15", "vidi7b"])
def test_the_greedy_continuation_has_rank_zero_and_the_inflight_logprobs(arch):
    s = setup(arch)
    toks, lps = s.model.generate_inflight([PROMPT, [2, 21, 22]], mm_state=s.mm, max_new_tokens=[6, 3], eos_token_id=999999, output_logprobs=True)
    off = s.model.generate_inflight([PROMPT, [2, 21, 22]], mm_state=s.mm, max_new_tokens=[6, 3], eos_token_id=999999)
    assert [t.tolist() for t in toks] == [t.tolist() for t in off] and [len(t) for t in toks] == [6, 3]
    assert all(v.dtype == torch.float32 and v.shape == t.shape and bool((v <= 0).all()) for t, v in zip(toks, lps))
    for p, t, v in zip([PROMPT, [2, 21, 22]], toks, lps):
        rec = s.model.score(p, [t], mm_state=s.mm)[0]
        assert rec.ranks.tolist() == [0] * len(t)
        assert float((rec.token_logprobs - v).abs().max()) <= PER_TOKEN


# ---------------------------------------------------------------------------------------------------------------------------------------
# the loop over the scripted engine
# ---------------------------------------------------------------------------------------------------------------------------------------
def value(pid, step):
    return -(pid + step / 64.0)                                     # exact in fp32


class FakeLogprobEngine(FakeEngine):
    def token_logprobs(self, hid):
        self.calls.append(("logprobs", len(hid)))
        return [token(pid, step) for pid, step in hid], [value(pid, step) for pid, step in hid], [0] * len(hid)

    def logits_argmax(self, hid):
        raise AssertionError("with logprobs=True the loop asks token_logprobs")


def test_run_inflight_logprobs_line_up_with_the_tokens():
    prompts = make_prompts(6)
    eos = [token(3, 2), token(5, 0)]                                 # prompt 3 ends on EOS at its third token, prompt 5 at its admission prefill
    max_new = [6, 1, 6, 6, 6, 4]                                     # prompt 2 is complete after its prefill token as well
    eng = FakeLogprobEngine()
    out, lps = run_inflight(eng, prompts, None, max_new, eos_ids=eos, max_rows=2, min_admit=1, logprobs=True)
    assert out == [expected(p[0], m, eos) for p, m in zip(prompts, max_new)]
    assert [len(o) for o in out] == [6, 1, 3, 6, 1, 4]
    assert lps == [[value(p[0], st) for st in range(len(o))] for p, o in zip(prompts, out)]
    steps = [c for c in eng.calls if c[0] in ("prefill", "decode")]
    assert len([c for c in eng.calls if c[0] == "logprobs"]) == len(steps)          # one decision, so one host copy, per step
    assert run_inflight(eng, [], None, [], logprobs=True) == ([], [])


def test_flag_off_needs_no_token_logprobs():
    eng = FakeEngine()
    assert not hasattr(eng, "token_logprobs")
    prompts = make_prompts(5)
    out = run_inflight(eng, prompts, None, [3] * 5, max_rows=2)
    assert out == [expected(p[0], 3) for p in prompts]
    with pytest.raises(AttributeError):
        run_inflight(eng, prompts, None, [3] * 5, max_rows=2, logprobs=True)
    s = setup("vidi15")
    assert all(torch.is_tensor(t) for t in s.model.generate_inflight([PROMPT], mm_state=s.mm, max_new_tokens=2))      # a list of tensors, no tuple
    with pytest.raises(NotImplementedError):                        # an engine with slots but without the method
        from vidi_amd.model import VidiForCausalLM
        VidiForCausalLM(s.cfg, s.eng.w, dtype=torch.float32, device="cpu", engine=InflightOracleEngine(s.cfg, s.eng.w)).generate_inflight(
            [PROMPT], mm_state=s.mm, max_new_tokens=2, output_logprobs=True)


def test_refusals():
    from vidi_amd.engine import MMBatchState
    s = setup("vidi15")
    assert len(s.model.score(PROMPT, s.cands[:1], mm_state=s.mm)) == 1
    with pytest.raises(NotImplementedError, match="ONE resident video"):
        s.model.score(PROMPT, s.cands, mm_state=MMBatchState.__new__(MMBatchState))
    s.eng.world = 2
    try:
        with pytest.raises(NotImplementedError, match="sharded"):
            s.model.score(PROMPT, s.cands, mm_state=s.mm)
    finally:
        s.eng.world = 1
    with pytest.raises(ValueError):
        s.model.score(PROMPT, [s.cands[0], []], mm_state=s.mm)
    with pytest.raises(ValueError):
        s.model.score([-200], s.cands, mm_state=s.mm)               # nothing in front of the first candidate token
    assert s.eng.forwards == [(1, 6)]                                # a refused call runs nothing


# ---------------------------------------------------------------------------------------------------------------------------------------
# the C ABI's argument checks: before any launch, so without a GPU
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_token_logprob_argument_validation_without_gpu():
    from vidi_amd import hip
    from vidi_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    fn = lib.vidi_token_logprob
    fn.restype, fn.argtypes = ctypes.c_int, hip.SIGNATURES["vidi_token_logprob"]
    per_row = hip.TOKEN_LOGPROB_WORKSPACE_BYTES_PER_ROW
    assert per_row == 2048
    R, V = 3, 64
    ptr = 0x10000                                                    # never dereferenced on the host: every case below returns before a launch
    call = lambda **kw: fn(*[{**dict(logits=ptr, targets=None, idx=ptr, lse=ptr, logprob=ptr, rank=ptr, R=R, V=V, ld=V, cap=30.0, dtype=0, ws=ptr,  # noqa: E731
                                     ws_bytes=R * per_row, stream=None), **kw}[k]
                             for k in ("logits", "targets", "idx", "lse", "logprob", "rank", "R", "V", "ld", "cap", "dtype", "ws", "ws_bytes", "stream")])
    for name in ("logits", "idx", "lse", "logprob", "rank", "ws"):
        assert call(**{name: None}) == -4, name                      # VIDI_ERR_ARG
    assert call(ws=ptr + 8) == -3                                    # VIDI_ERR_ALIGN: 16 bytes
    assert call(ws_bytes=R * per_row - 1) == -1                      # VIDI_ERR_SHAPE: too small for R rows
    assert call(R=0) == -1 and call(V=0) == -1 and call(ld=V - 1) == -1
    assert call(dtype=2) == -2
