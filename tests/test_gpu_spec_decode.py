"""Prompt-lookup speculative decoding on the GPU: a verify step (5 and 16 rows on a filled text cache) + cache roll-back of the HIP engine
against the CPU oracle engine, and `generate(prompt_lookup_num_tokens=...)` against the same engine's plain greedy run."""
import pytest
import torch

from test_gpu_multivideo import new_model, timed
from test_spec_decode import PROMPT, SpecOracleEngine
from util import logit_tol, report, seeded

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. the engine: a verify step, the roll-back and the step after it against the CPU oracle engine
# ---------------------------------------------------------------------------------------------------------------------------------------
LONG_PROMPT = [2, 21, 22, -200] + list(range(30, 48))          # 21 text positions: tiny's sliding window (16) ends inside the prompt
STEPS = {5: [50, 51, 52, 53, 54], 16: list(range(50, 66))}      # 16 rows: the most a verify step carries at G = 2 (spec_max_draft() + 1)
AFTER = 70


def video(cfg, dt, dev):
    S = cfg.vis_image_size
    px = seeded((2, 3, S, S), 702, 0.5).clamp(-1, 1).to(dt).to(dev)
    mel = seeded((1, cfg.aud_num_mel_bins, cfg.aud_nb_max_frames), 710, 0.3).to(dt).to(dev)
    return [px], [mel], [100]


def verify_then_roll_back(model, mm, n):
    """prefill, one Lq = n step on given tokens, keep 2 of the n, one Lq = 1 step -> (logits [n, V], logits [1, V], the text state)"""
    from vidi_amd.model import strip_image_token
    eng = model.engine
    ids, mask, pos = strip_image_token(torch.tensor([LONG_PROMPT], dtype=torch.int64), None)
    ts, _ = model._prefill(ids, mask, pos, mm, 18)
    p0, nv0 = ts.past_len, ts.n_valid.clone()
    posn = nv0[0] + torch.arange(n, dtype=torch.int64, device=eng.dev)
    ts.n_valid += n
    hn = eng.text_forward(eng.embed_tokens(torch.tensor(STEPS[n], dtype=torch.int64, device=eng.dev)), posn, ts, mm, Lq=n)
    l5 = eng.logits_argmax(hn)[0].float().cpu().clone()
    assert ts.past_len == p0 + n
    eng.truncate_text_state(ts, p0 + 2)
    assert ts.past_len == p0 + 2 and ts.n_valid.tolist() == (nv0 + 2).tolist()
    posn = ts.n_valid.clone()
    ts.n_valid += 1
    hn = eng.text_forward(eng.embed_tokens(torch.tensor([AFTER], dtype=torch.int64, device=eng.dev)), posn, ts, mm, Lq=1)
    l1 = eng.logits_argmax(hn)[0].float().cpu().clone()
    return l5, l1, ts


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("arch", ["tiny", "tiny_7b"])
@pytest.mark.parametrize("n", [5, 16])
def test_engine_verify_step_and_roll_back_against_the_oracle(n, arch, dt):
    from vidi_amd import config
    from vidi_amd.model import VidiForCausalLM
    cfg = getattr(config, arch)()
    model, w32 = new_model(cfg, dt, seed=3)
    om = VidiForCausalLM(cfg, w32, dtype=torch.float32, device="cpu", engine=SpecOracleEngine(cfg, w32))
    r5, r1, _ = verify_then_roll_back(om, om.encode_mm_state(*video(cfg, torch.float32, "cpu")), n)
    mm = model.encode_mm_state(*video(cfg, dt, "cuda"))
    (l5, l1, ts), names = timed(lambda: verify_then_roll_back(model, mm, n))
    assert names.count("vidi_attn_text") >= 2 * cfg.num_hidden_layers          # prefill and verify step: vidi_rope_cache + vidi_attn_text per layer
    report(f"verify step, {n} logit rows", l5, r5, logit_tol(dt, r5), 0.0)
    report("the step after the roll-back", l1, r1, logit_tol(dt, r1), 0.0)
    p0 = len(LONG_PROMPT) - 1
    assert ts.kmask[0].tolist() == [1] * (p0 + 3) + [0] * (ts.Lmax - p0 - 3) and int(ts.n_valid[0]) == p0 + 3


def test_engine_roll_back_bookkeeping():
    """truncate_text_state: past_len, the mask bytes of the dropped slots and n_valid; the K/V rows stay; growing is refused"""
    from vidi_amd.config import tiny
    model, _ = new_model(tiny(), torch.bfloat16, seed=3)
    eng = model.engine
    assert eng.spec_max_draft() == 15
    ts = eng.new_text_state(2, 12)
    ts.kmask[:, :7] = 1
    ts.kmask[1, 5] = 0
    ts.past_len, ts.n_valid = 7, torch.tensor([7, 6], device="cuda")
    ts.kc.fill_(1.0)
    eng.truncate_text_state(ts, 4)
    assert ts.past_len == 4 and ts.n_valid.tolist() == [4, 4] and ts.kmask.sum(-1).tolist() == [4, 4] and float(ts.kc.min()) == 1.0
    with pytest.raises(ValueError):
        eng.truncate_text_state(ts, 5)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 7. generate()
# ---------------------------------------------------------------------------------------------------------------------------------------
N_NEW, K = 9, 3
# (config, weight seed): chosen on the CPU oracle (the video / prompt of tests/test_spec_decode.py): the plain run's top-2 margin exceeds
# 2 x logit_tol(bf16) on its first 6 (Vidi1.5, untied head: tied random embeddings echo their input) / all 9 (Vidi-7B) steps, and the tokens vary
GEN_CASES = {"vidi15": (dict(tie_word_embeddings=False), 8), "vidi7b": ({}, 8)}


class Streamer:
    def __init__(self):
        self.got, self.ended = [], False

    def put(self, t):
        self.got.extend(t.reshape(-1).tolist())

    def end(self):
        self.ended = True


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("arch", ["vidi15", "vidi7b"])
def test_generate_with_drafts_against_plain_greedy(arch, dt):
    from vidi_amd import config
    over, seed = GEN_CASES[arch]
    cfg = (config.tiny if arch == "vidi15" else config.tiny_7b)(**over)
    model, _ = new_model(cfg, dt, seed=seed)
    eng = model.engine
    mm = model.encode_mm_state(*video(cfg, dt, "cuda"))
    ids = torch.tensor([PROMPT], dtype=torch.int64)
    gen = lambda **kw: model.generate(ids, mm_state=mm, max_new_tokens=N_NEW, eos_token_id=999999, **kw)      # noqa: E731
    full = gen(return_dict_in_generate=True, output_logits=True)
    plain = full.sequences[0].tolist()
    assert plain == gen()[0].tolist() and len(plain) == N_NEW
    logits = torch.cat([l.float().cpu() for l in full.logits])
    ltol = logit_tol(dt, logits)
    margin = [float(torch.topk(l, 2).values.diff().abs()) for l in logits]
    n_cmp = next((t for t, m in enumerate(margin) if m <= 2 * ltol), N_NEW)        # tokens are compared up to the first low-margin step of the plain run
    print(f"{arch}: plain {plain}; margins {[round(m, 3) for m in margin]} against 2 x tol = {2 * ltol:.3f}: the first {n_cmp} tokens are compared")
    assert 2 * n_cmp >= N_NEW, "fewer than half of the positions are compared: pick other seeds"
    n_prompt = len(PROMPT) - 1

    def forced(wrong_at=()):
        def draft(history, k, max_ngram, eos_ids):
            n_new = len(history) - n_prompt
            d = plain[n_new: n_new + k]
            return [(t + 1) % cfg.vocab_size if i in wrong_at else t for i, t in enumerate(d)]
        return draft

    lqs = []
    inner = eng.text_forward

    def recording(hidden, positions, ts, mm_, Lq, **kw):
        lqs.append((ts.past_len, Lq))
        return inner(hidden, positions, ts, mm_, Lq, **kw)
    eng.text_forward = recording
    try:
        for name, fn in (("oracle", forced()), ("wrong", forced((0, 1, 2))), ("mixed", forced((2,))), ("lookup", None)):
            model.__dict__.pop("_spec_draft", None)
            if fn is not None:
                model._spec_draft = fn
            del lqs[:]
            st = Streamer()
            got, names = timed(lambda: gen(prompt_lookup_num_tokens=K, streamer=st))
            got = got[0].tolist()
            print(f"{arch} {name} drafts: {got}; (cache length, rows) per text_forward {lqs}")
            assert got[:n_cmp] == plain[:n_cmp], (name, got, plain)
            assert st.got == got and st.ended
            assert any(lq > 1 for p0, lq in lqs if p0 > 0), name                 # (lookup: the seeds were chosen so that a draft occurs)
            assert "vidi_attn_text" in names and "vidi_rope_cache" in names
            if name == "oracle":
                # the first verify step's first draft is plain[1]; got[1] is that step's first argmax: equal inside the compared prefix = accepted ...
                assert n_cmp >= 2 and lqs[1] == (n_prompt, K + 1) and got[1] == plain[1]
                if got == plain:
                    assert [lq for _, lq in lqs[1:]] == [4, 4]             # ... and with every draft accepted 1 + 4 + 4 tokens take two steps
    finally:
        del eng.text_forward
        model.__dict__.pop("_spec_draft", None)
