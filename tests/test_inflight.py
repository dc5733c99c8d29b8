"""In-flight batching on the CPU: the scheduler (vidi_amd/inflight.py) over a scripted fake engine that records every call, and
`generate_inflight()` over the CPU oracle engine — the tokens of the per-prompt plain `generate()`, exactly."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
sys.path.insert(0, HERE)

from oracle_engine import OracleEngine  # noqa: E402
from util import seeded  # noqa: E402
from vidi_amd.inflight import run_inflight, simulate_steps, static_batch_steps  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the scheduler over a scripted engine
# ---------------------------------------------------------------------------------------------------------------------------------------
def token(pid, step):
    """the scripted model: token `step` (0 = the prefill's) of the prompt whose first id is `pid`"""
    return 100 + (pid * 37 + step * 11) % 800


class FakeEngine:
    """slots hold (prompt id, tokens cached); a 'hidden state' is the list of (prompt id, step) whose token the argmax then yields"""

    def __init__(self, rows=4):
        self.rows, self.calls, self.slots = rows, [], None

    def max_inflight_rows(self):
        return self.rows

    def new_text_slots(self, S, Lmax):
        self.slots = SimpleNamespace(S=S, Lmax=Lmax, length=[-1] * S, pid=[None] * S, n0=[0] * S)
        self.calls.append(("new", S, Lmax))
        return self.slots

    def slots_prefill(self, slots, slot_ids, prompts, mm):
        assert slots is self.slots and len(slot_ids) == len(prompts) == len(set(slot_ids)) > 0
        self.calls.append(("prefill", list(slot_ids), [p[0] for p in prompts]))
        hid = []
        for s, p in zip(slot_ids, prompts):
            assert slots.length[s] == -1, f"slot {s} admitted while in use"
            slots.length[s], slots.pid[s], slots.n0[s] = len(p), p[0], len(p)
            hid.append((p[0], 0))
        return hid

    def slots_decode(self, slots, slot_ids, token_ids, mm):
        assert len(slot_ids) == len(token_ids) == len(set(slot_ids)) > 0
        self.calls.append(("decode", list(slot_ids), [slots.pid[s] for s in slot_ids]))
        hid = []
        for s, t in zip(slot_ids, token_ids):
            assert 0 <= slots.length[s] < slots.Lmax, f"slot {s} decoded while free or full"
            step = slots.length[s] - slots.n0[s]                    # tokens fed so far = index of the token being fed
            assert t == token(slots.pid[s], step), "the loop must feed the token it was given last"
            slots.length[s] += 1
            hid.append((slots.pid[s], step + 1))
        return hid

    def logits_argmax(self, hid):
        return None, [token(pid, step) for pid, step in hid]


def make_prompts(n):
    return [[i + 1] + [5] * (i % 4) for i in range(n)]              # first id = prompt id; lengths 1..4


def expected(pid, n_new, eos=()):
    out = []
    for st in range(n_new):
        out.append(token(pid, st))
        if out[-1] in eos:
            break
    return out


MAX_NEW = [5, 1, 9, 3, 1, 7, 2, 12, 4, 6, 1, 8]


def replay(calls, prompts, results):
    """walk the recorded calls -> per decode call: (rows carried, prompts not finished before it, prompts waiting before it); also checks that
    no two live prompts share a slot and that a prompt's rows are contiguous in time"""
    n_out = {p[0]: len(r) for p, r in zip(prompts, results)}
    got = {p[0]: 0 for p in prompts}
    owner, admitted, rec = {}, set(), []
    for kind, sl, pids in [c for c in calls if c[0] != "new"]:
        if kind == "prefill":
            for s, pid in zip(sl, pids):
                assert s not in owner, f"slot {s} handed out twice"
                assert pid not in admitted
                admitted.add(pid)
                got[pid] = 1
                if got[pid] < n_out[pid]:
                    owner[s] = pid
        else:
            unfinished = sum(1 for pid in got if got[pid] < n_out[pid])
            waiting = len(prompts) - len(admitted)
            assert sorted(sl) == sorted(owner) and [owner[s] for s in sl] == pids, "a decode call carries exactly the live rows"
            rec.append((len(sl), unfinished, waiting))
            for s in sl:
                got[owner[s]] += 1
                if got[owner[s]] == n_out[owner[s]]:
                    del owner[s]
    assert not owner and got == n_out
    return rec


def test_results_in_input_order_and_per_prompt_lengths():
    eng = FakeEngine()
    prompts = make_prompts(len(MAX_NEW))
    out = run_inflight(eng, prompts, "mm", MAX_NEW, max_rows=3, min_admit=1)
    assert out == [expected(p[0], m) for p, m in zip(prompts, MAX_NEW)]
    assert eng.calls[0] == ("new", 3, 4 + 12)                        # Lmax = longest prompt + largest max_new


def test_eos_cuts_the_answer_and_is_included():
    prompts = make_prompts(6)
    eos = [token(3, 2), token(5, 0)]                                 # prompt 3 stops at its third token, prompt 5 at its prefill token
    eng = FakeEngine()
    out = run_inflight(eng, prompts, None, [6] * 6, eos_ids=eos, max_rows=2, min_admit=1)
    want = [expected(p[0], 6, eos) for p in prompts]
    assert out == want and len(want[2]) == 3 and want[2][-1] == eos[0] and want[4] == [eos[1]]
    assert all(5 not in pids for kind, _, pids in eng.calls[1:] if kind == "decode")     # finished at its prefill: never a decode row


def test_a_prompt_with_one_new_token_never_occupies_a_decode_row():
    eng = FakeEngine()
    prompts = make_prompts(len(MAX_NEW))
    run_inflight(eng, prompts, None, MAX_NEW, max_rows=3, min_admit=1)
    ones = {p[0] for p, m in zip(prompts, MAX_NEW) if m == 1}
    assert len(ones) == 3
    assert not any(ones & set(pids) for kind, _, pids in eng.calls[1:] if kind == "decode")


@pytest.mark.parametrize("max_rows", [1, 3, 4, 16])
def test_min_admit_1_keeps_every_row_full(max_rows):
    """no slot idles while a prompt waits: every decode call carries min(max_rows, prompts not yet finished) rows"""
    eng = FakeEngine()
    prompts = make_prompts(len(MAX_NEW))
    out = run_inflight(eng, prompts, None, MAX_NEW, max_rows=max_rows, min_admit=1)
    rec = replay(eng.calls, prompts, out)
    assert rec and all(rows == min(max_rows, unfinished) for rows, unfinished, _ in rec), rec
    steps, rows, prefills = simulate_steps(MAX_NEW, max_rows, 1)
    assert (steps, rows) == (len(rec), sum(r for r, _, _ in rec)) and rows == sum(m - 1 for m in MAX_NEW)
    assert prefills == sum(1 for c in eng.calls if c[0] == "prefill")


def test_a_freed_slot_is_reused_and_never_shared():
    eng = FakeEngine()
    prompts = make_prompts(len(MAX_NEW))
    out = run_inflight(eng, prompts, None, MAX_NEW, max_rows=2, min_admit=1)
    replay(eng.calls, prompts, out)                                  # asserts: no slot handed out while owned
    used = [s for kind, sl, _ in eng.calls[1:] if kind == "prefill" for s in sl]
    assert set(used) == {0, 1} and len(used) == len(prompts)         # 12 prompts went through 2 slots


def test_min_admit_3_delays_admissions():
    eng = FakeEngine()
    prompts = make_prompts(len(MAX_NEW))
    out = run_inflight(eng, prompts, None, MAX_NEW, max_rows=4, min_admit=3)
    assert out == [expected(p[0], m) for p, m in zip(prompts, MAX_NEW)]
    rec = replay(eng.calls, prompts, out)
    # an admission (after the first) happens only with >= min(3, waiting) free slots, or with no live row
    live, n_wait = set(), len(prompts)
    n_out = {p[0]: len(r) for p, r in zip(prompts, out)}
    got = {}
    delayed = 0
    for kind, sl, pids in eng.calls[1:]:
        if kind == "prefill":
            free_before = 4 - len(live)
            assert free_before >= min(3, n_wait) or not live, (free_before, n_wait, live)
            assert len(sl) == min(free_before, n_wait)               # all free slots are filled by ONE call
            n_wait -= len(sl)
            for s, pid in zip(sl, pids):
                got[pid] = 1
                if n_out[pid] > 1:
                    live.add(s)
        else:
            if n_wait and len(sl) < 4:
                delayed += 1                                         # a step ran with a free slot while a prompt waited
            for s, pid in zip(sl, pids):
                got[pid] += 1
                if got[pid] == n_out[pid]:
                    live.discard(s)
    assert delayed > 0
    assert any(rows < min(4, unfinished) for rows, unfinished, waiting in rec if waiting)
    assert (len(rec), sum(r for r, _, _ in rec)) == simulate_steps(MAX_NEW, 4, 3)[:2]
    assert sum(1 for c in eng.calls if c[0] == "prefill") < sum(1 for c in FakeRun(4, 1).calls if c[0] == "prefill")


def FakeRun(max_rows, min_admit):
    eng = FakeEngine()
    run_inflight(eng, make_prompts(len(MAX_NEW)), None, MAX_NEW, max_rows=max_rows, min_admit=min_admit)
    return eng


def test_on_finish_fires_once_per_prompt_in_completion_order():
    eng = FakeEngine()
    prompts = make_prompts(len(MAX_NEW))
    seen = []
    out = run_inflight(eng, prompts, None, MAX_NEW, max_rows=3, min_admit=1, on_finish=lambda i, toks: seen.append((i, toks)))
    assert sorted(i for i, _ in seen) == list(range(len(prompts)))
    assert all(toks == out[i] for i, toks in seen)
    assert [i for i, _ in seen] != list(range(len(prompts)))        # short answers admitted later overtake long ones


def test_step_models():
    assert static_batch_steps([5, 2, 9, 3], 2) == (4 + 8, 8 + 16, 2)
    assert simulate_steps([5, 2, 9, 3], 2, 1) == (9, 4 + 1 + 8 + 2, 3)
    assert simulate_steps([1, 1, 1], 2, 1) == (0, 0, 2)


def test_bad_arguments():
    eng = FakeEngine()
    with pytest.raises(ValueError):
        run_inflight(eng, [[1], [2]], None, [3])
    with pytest.raises(ValueError):
        run_inflight(eng, [[1]], None, [0])
    with pytest.raises(ValueError):
        run_inflight(eng, [[1]], None, [2], max_rows=0)
    assert run_inflight(eng, [], None, []) == []


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. generate_inflight() over the oracle engine
# ---------------------------------------------------------------------------------------------------------------------------------------
class InflightOracleEngine(OracleEngine):
    """the oracle engine + text-cache slots: every slot is an independent ONE-ROW oracle state, so a prompt's numbers are those of its own
    plain run whatever shares the step with it; records the slot calls and the top-2 margins"""

    def __init__(self, cfg, w):
        super().__init__(cfg, w)
        self.slot_calls, self.margins = [], []

    def max_inflight_rows(self):
        return 32 // (self.cfg.num_attention_heads // self.cfg.num_key_value_heads)

    def new_text_slots(self, S, Lmax):
        return SimpleNamespace(S=S, Lmax=Lmax, length=[-1] * S, states=[None] * S)

    def slots_prefill(self, slots, slot_ids, prompts, mm):
        self.slot_calls.append(("prefill", list(slot_ids), [len(p) for p in prompts]))
        last = []
        for s, p in zip(slot_ids, prompts):
            assert slots.length[s] == -1
            ts = self.new_text_state(1, slots.Lmax)
            ids = torch.tensor([int(t) for t in p], dtype=torch.int64)
            hn = self.text_forward(self.embed_tokens(ids), torch.arange(len(p)), ts, mm, Lq=len(p))
            slots.states[s], slots.length[s] = ts, len(p)
            last.append(hn[-1])
        return torch.stack(last)

    def slots_decode(self, slots, slot_ids, token_ids, mm):
        self.slot_calls.append(("decode", list(slot_ids), [slots.length[s] for s in slot_ids]))
        out = []
        for s, t in zip(slot_ids, token_ids):
            assert 0 <= slots.length[s] < slots.Lmax
            hn = self.text_forward(self.embed_tokens(torch.tensor([int(t)])), torch.tensor([slots.length[s]]), slots.states[s], mm, Lq=1)
            slots.length[s] += 1
            out.append(hn[0])
        return torch.stack(out)

    def logits_argmax(self, hn_last):
        logits, idx = super().logits_argmax(hn_last)
        top2 = torch.topk(logits.float(), 2, dim=-1).values
        self.margins.extend((top2[:, 0] - top2[:, 1]).tolist())
        return logits, idx


# 7 prompts of 3..21 text positions (tiny's 16-token sliding window ends inside the longer ones); the second holds the <image> placeholder
PROMPTS = [[2, 21, 22], [2, 30, -200, 31, 32, 33], list(range(40, 49)), list(range(60, 72)), list(range(80, 95)), list(range(100, 118)), list(range(130, 151))]
NEW = [6, 1, 9, 3, 12, 5, 8]
SEEDS = {"vidi15": 4, "vidi7b": 2}                                  # tests/test_spec_decode.py's (untied head for Vidi1.5: tied random embeddings echo their input)
_cache = {}


def setup(arch):
    if arch not in _cache:
        from vidi_amd.config import tiny, tiny_7b
        from vidi_amd.model import VidiForCausalLM
        from vidi_amd.weights import init_random_weights
        cfg = tiny(tie_word_embeddings=False) if arch == "vidi15" else tiny_7b()
        w = init_random_weights(cfg, seed=SEEDS[arch], dtype=torch.float32, device="cpu")
        eng = InflightOracleEngine(cfg, w)
        model = VidiForCausalLM(cfg, w, dtype=torch.float32, device="cpu", engine=eng)
        S = cfg.vis_image_size
        mm = model.encode_mm_state(seeded((2, 3, S, S), 702, 0.5).clamp(-1, 1)[None], seeded((1, cfg.aud_num_mel_bins, cfg.aud_nb_max_frames), 710, 0.3)[None], [100])
        plain = [model.generate(torch.tensor([p]), mm_state=mm, max_new_tokens=n, eos_token_id=999999)[0].tolist() for p, n in zip(PROMPTS, NEW)]
        _cache[arch] = SimpleNamespace(cfg=cfg, eng=eng, model=model, mm=mm, plain=plain)
    s = _cache[arch]
    s.eng.slot_calls = []
    return s


@pytest.mark.parametrize("arch", ["vidi15", "vidi7b"])
def test_generate_inflight_equals_per_prompt_plain_generate(arch):
    s = setup(arch)
    assert [len(p) for p in s.plain] == NEW and len({tuple(p[:3]) for p in s.plain}) > 2, "the plain runs should differ: pick another seed"
    seen = []
    got = s.model.generate_inflight([torch.tensor(p) for p in PROMPTS], mm_state=s.mm, max_new_tokens=NEW, eos_token_id=999999, max_rows=3,
                                    min_admit=1, on_finish=lambda i, t: seen.append((i, t.tolist())))
    assert [g.tolist() for g in got] == s.plain
    assert sorted(seen) == sorted(enumerate(s.plain))
    dec = [c for c in s.eng.slot_calls if c[0] == "decode"]
    assert max(len(c[1]) for c in dec) == 3 and len({tuple(c[2]) for c in dec if len(c[1]) == 3}) > 1
    assert any(len(set(c[2])) == len(c[2]) > 1 for c in dec), "rows of a step sit at different cache lengths"
    assert any(max(c[2]) > s.cfg.sliding_window for c in dec) or s.cfg.sliding_window > 64
    assert s.eng.slot_calls[0] == ("prefill", [0, 1, 2], [3, 5, 9])      # the placeholder is no text position
    # lists and min_admit go through as well; an EOS ends a prompt early, and is included
    eos = s.plain[4][5]
    at = s.plain[4].index(eos)
    got = s.model.generate_inflight(PROMPTS, mm_state=s.mm, max_new_tokens=NEW, eos_token_id=[999999, eos], max_rows=3, min_admit=2)
    for g, p in zip(got, s.plain):
        assert g.tolist() == (p[: p.index(eos) + 1] if eos in p else p)
    assert len(got[4]) == at + 1
    assert [g.tolist() for g in s.model.generate_inflight(PROMPTS[:2], mm_state=s.mm, max_new_tokens=3, eos_token_id=999999)] == \
        [s.model.generate(torch.tensor([p]), mm_state=s.mm, max_new_tokens=3, eos_token_id=999999)[0].tolist() for p in PROMPTS[:2]]


def test_refusals():
    s = setup("vidi15")
    gen = lambda **kw: s.model.generate_inflight(PROMPTS[:2], mm_state=kw.pop("mm", s.mm), max_new_tokens=2, **kw)      # noqa: E731
    assert len(gen()) == 2
    for kw in (dict(do_sample=True), dict(num_beams=2), dict(logits_processor=[lambda i, x: x]), dict(repetition_penalty=1.3),
               dict(no_repeat_ngram_size=2), dict(stopping_criteria=[lambda i, x: False]), dict(max_time=5.0), dict(return_dict_in_generate=True),
               dict(prompt_lookup_num_tokens=3), dict(typical_p=0.5)):
        with pytest.raises(NotImplementedError):
            gen(**kw)
    from vidi_amd.engine import MMBatchState
    with pytest.raises(NotImplementedError):
        gen(mm=MMBatchState.__new__(MMBatchState))
    s.eng.world = 2
    try:
        with pytest.raises(NotImplementedError):
            gen()
    finally:
        s.eng.world = 1
    from vidi_amd.model import VidiForCausalLM
    m2 = VidiForCausalLM(s.cfg, s.eng.w, dtype=torch.float32, device="cpu", engine=OracleEngine(s.cfg, s.eng.w))   # no slot methods
    with pytest.raises(NotImplementedError):
        m2.generate_inflight(PROMPTS[:2], mm_state=s.mm, max_new_tokens=2)
