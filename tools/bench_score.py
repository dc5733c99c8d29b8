"""Per-token log-probabilities: what the vocabulary pass, `score()` and `generate_inflight(output_logprobs=True)` cost -> profiles/score_logprobs.json.

  python tools/bench_score.py [--frames 3600] [--rounds 5] [--out profiles/score_logprobs.json]

(a) kernel   vidi_token_logprob (both launches) at V = 256 000 for R = 1, 16, 256 rows in bf16 and fp16, beside vidi_softcap_argmax (on a copy: it
             writes in place) and beside torch's `log_softmax(logits.float())` + gather on the same tensor (no softcap in that arm).  Each arm
             is captured once as a hipGraph of `--iters` back-to-back calls, so a window (two device events around one replay) holds device
             time and not the host's launch rate; the arms alternate inside a round; round 0 is dropped.  For R = 1 and 16 the run also
             records max |lse or logprob - fp64|, fp64 computed on the CPU from the values vidi_softcap_argmax leaves in a copy (the bound of
             tests/test_gpu_score.py is 5e-5).
(b) score()  16 candidates x 16 tokens behind one 39-token prompt on the 60-minute caches of bench.py (Vidi1.5-9B decoder, random weights, bf16),
             against a loop of 16 `forward(labels=...)` calls with the labels masked to the candidate, and against score() with
             `max_positions` = one row (one candidate per prefill: the forward loop's prefill width, so what is left is the vocabulary pass): wall time (device events around a run that
             ends in a synchronise) and torch.cuda.max_memory_allocated above what is resident, arms alternating; and the largest difference
             between the two arms' per-candidate sums.
(c) in-flight  tools/bench_inflight.py's workload (64 prompts, 8..128 new tokens, no EOS) with and without `output_logprobs`, arms alternating.
Spread = (max - min) / mean over the kept rounds of an arm; the largest per section is stated."""
import argparse
import dataclasses
import json
import os
import random
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V = 256000
CAP = 30.0


def stats(v):
    mean = sum(v) / len(v)
    return dict(mean=round(mean, 4), min=round(min(v), 4), max=round(max(v), 4), spread=round((max(v) - min(v)) / mean, 4))


def window(fn, iters=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(arms, rounds, iters=1):
    """arms: [(name, fn)] -> {name: [ms per call, one per kept round]}; round 0 warms every arm and is dropped"""
    meas = {}
    for r in range(rounds + 1):
        for name, fn in arms:
            ms = window(fn, iters)
            if r:
                meas.setdefault(name, []).append(ms)
    return meas


def graphed(fn, iters):
    """`iters` back-to-back calls of fn as one captured graph -> its replay"""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    return g.replay


def kernel_section(hip, rounds, iters):
    rows = []
    for dt, dname in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
        for R in (1, 16, 256):
            g = torch.Generator(device="cuda").manual_seed(R)
            logits = (torch.rand((R, V), generator=g, device="cuda") * 60.0 - 30.0).to(dt)
            scratch = logits.clone()
            targets = torch.randint(0, V, (R,), generator=g, device="cuda")
            idx = torch.empty((R,), dtype=torch.int64, device="cuda")
            ws_lp, ws_am = hip.token_logprob_workspace(R, "cuda"), hip.softcap_argmax_workspace(R, "cuda")
            rec = dict(dtype=dname, R=R, V=V, logit_bytes=R * V * 2)
            if R <= 16:
                capped = logits.clone()
                hip.softcap_argmax(capped, idx, CAP, ws_am)
                x = capped.cpu().double()
                lse64 = torch.logsumexp(x, dim=-1)
                lp64 = x.gather(1, targets.cpu()[:, None])[:, 0] - lse64
                _, lse, lp, _ = hip.token_logprob(logits, targets, CAP, ws_lp)
                rec["max_abs_error_vs_fp64"] = float(max((lse.cpu().double() - lse64).abs().max(), (lp.cpu().double() - lp64).abs().max()))
                del capped
            arms = [("vidi_token_logprob", lambda: hip.token_logprob(logits, targets, CAP, ws_lp)),
                    ("vidi_softcap_argmax", lambda: hip.softcap_argmax(scratch, idx, CAP, ws_am)),
                    ("torch log_softmax(float) + gather", lambda: torch.log_softmax(logits.float(), dim=-1).gather(1, targets[:, None]))]
            meas = alternate([(name, graphed(fn, iters)) for name, fn in arms], rounds)
            for name, v in meas.items():
                s = stats([x / iters for x in v])
                rec[name] = dict(us=round(s["mean"] * 1e3, 2), min_us=round(s["min"] * 1e3, 2), max_us=round(s["max"] * 1e3, 2), spread=s["spread"])
            rec["read_GB_per_s"] = round(R * V * 2 / (rec["vidi_token_logprob"]["us"] * 1e-6) / 1e9, 1)
            rows.append(rec)
            del logits, scratch
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3600)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50, help="calls per timed window of the kernel section")
    ap.add_argument("--prompts", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "score_logprobs.json"))
    a = ap.parse_args()
    from vidi_amd import config as C
    from vidi_amd import hip
    from vidi_amd.engine import VidiEngine
    from vidi_amd.model import VidiForCausalLM
    from vidi_amd.weights import init_random_weights
    if not torch.cuda.is_available():
        raise SystemExit("bench_score needs the GPU: a CPU run says nothing about a kernel's time")
    hip.load_library()

    dt = torch.bfloat16
    cfg = dataclasses.replace(C.vidi15_9b(), vis_num_layers=1, aud_num_layers=1)        # the towers are not part of a text pass
    eng = VidiEngine(cfg, init_random_weights(cfg, seed=3, dtype=dt, device="cuda"), dtype=dt, device="cuda")
    model = VidiForCausalLM(cfg, {}, dtype=dt, device="cuda", engine=eng)
    g = torch.Generator(device="cuda").manual_seed(5)
    n_img, n_aud = 25 * a.frames, 10 * a.frames
    img = (torch.randn((n_img, cfg.hidden_size), generator=g, device="cuda") * cfg.mm_std * eng.normalizer).to(dt)
    aud = (torch.randn((n_aud, cfg.hidden_size), generator=g, device="cuda") * cfg.mm_std * eng.normalizer).to(dt)
    mm = eng.mm_stream_prefill(img, None, aud, None, pre_normalized=True, check_masks=False)
    mm.img_any_valid = mm.aud_any_valid = True
    del img, aud

    # ---- (b) score() against the forward(labels=...) loop ----
    L, NC, LC = 39, 16, 16
    cpu = torch.Generator().manual_seed(7)
    prompt = torch.randint(0, cfg.vocab_size, (L,), generator=cpu)
    cands = [torch.randint(0, cfg.vocab_size, (LC,), generator=cpu) for _ in range(NC)]
    got = {}

    def arm_score():
        got["score"] = [r.logprob for r in model.score(prompt, cands, mm_state=mm)]

    def arm_forward():
        out = []
        for c in cands:
            ids = torch.cat([prompt, c])[None]
            labels = torch.cat([torch.full((L,), -100, dtype=torch.int64), c])[None]
            out.append(model.forward(ids, mm_state=mm, labels=labels).loss)
        got["forward"] = [-float(x) * LC for x in out]

    peak = {}

    def with_peak(name, fn):
        def run():
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            peak[name] = dict(resident_bytes=base, peak_bytes=torch.cuda.max_memory_allocated(), above_resident_bytes=torch.cuda.max_memory_allocated() - base)
        return run

    def arm_score_one():
        got["score_one"] = [r.logprob for r in model.score(prompt, cands, mm_state=mm, max_positions=L + LC)]
    arms_b = [("score(): 16 candidates x 16 tokens", with_peak("score", arm_score)), ("16 x forward(labels=)", with_peak("forward", arm_forward)),
              ("score(max_positions=55): one candidate per prefill", with_peak("score_one", arm_score_one))]
    meas_b = alternate(arms_b, a.rounds)
    sec_b = dict(prompt_len=L, candidates=NC, candidate_len=LC, max_positions=512,
                 largest_difference_of_candidate_sums=round(max(abs(x - y) for x, y in zip(got["score"], got["forward"])), 5),
                 largest_difference_one_candidate_per_prefill=round(max(abs(x - y) for x, y in zip(got["score_one"], got["forward"])), 5),
                 mean_candidate_sum=round(sum(got["forward"]) / NC, 3), arms=[])
    for (name, _), key in zip(arms_b, ("score", "forward", "score_one")):
        sec_b["arms"].append(dict(arm=name, wall_ms=stats(meas_b[name]), **peak[key]))
    sec_b["speedup"] = round(sec_b["arms"][1]["wall_ms"]["mean"] / sec_b["arms"][0]["wall_ms"]["mean"], 3)

    # ---- (c) the in-flight loop with and without output_logprobs ----
    N = a.prompts
    rng = random.Random(11)
    lengths = [rng.randint(8, 128) for _ in range(N)]
    base = torch.randint(0, cfg.vocab_size, (L,), generator=g, device="cuda").cpu()
    prompts = base.repeat(N, 1)
    prompts[:, -4:] = torch.randint(0, cfg.vocab_size, (N, 4), generator=torch.Generator().manual_seed(7))
    no_eos = cfg.vocab_size + 7
    toks = {}

    def inflight(flag):
        def run():
            out = model.generate_inflight(list(prompts), mm_state=mm, max_new_tokens=lengths, eos_token_id=no_eos, output_logprobs=flag)
            toks[flag] = [t.tolist() for t in (out[0] if flag else out)]
        return run
    arms_c = [("generate_inflight()", inflight(False)), ("generate_inflight(output_logprobs=True)", inflight(True))]
    meas_c = alternate(arms_c, min(a.rounds, 3))
    sec_c = dict(prompts=N, prompt_len=L, useful_tokens=sum(lengths), max_rows=eng.max_inflight_rows(), same_tokens=toks[True] == toks[False],
                 arms=[dict(arm=name, wall_ms=stats(meas_c[name])) for name, _ in arms_c])
    sec_c["ratio_with_over_without"] = round(sec_c["arms"][1]["wall_ms"]["mean"] / sec_c["arms"][0]["wall_ms"]["mean"], 4)

    kernel = kernel_section(hip, a.rounds, a.iters)
    spread = lambda rows_: max(r_["spread"] for r_ in rows_)          # noqa: E731
    out = dict(what="per-token log-probabilities: the vocabulary pass, score() and the in-flight loop; see tools/bench_score.py",
               device=torch.cuda.get_device_name(0), preset="vidi15_9b (random weights)", frames=a.frames, image_keys=n_img, audio_keys=n_aud,
               rounds=a.rounds, kernel_iters_per_window=a.iters, final_logit_softcapping=CAP,
               max_abs_error_vs_fp64=dict(bound=5e-5, measured=max(r_["max_abs_error_vs_fp64"] for r_ in kernel if "max_abs_error_vs_fp64" in r_)),
               kernel=kernel, kernel_largest_spread=spread([r_[k] for r_ in kernel for k in r_ if isinstance(r_[k], dict)]),
               score=sec_b, score_largest_spread=spread([x["wall_ms"] for x in sec_b["arms"]]),
               inflight=sec_c, inflight_largest_spread=spread([x["wall_ms"] for x in sec_c["arms"]]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(dict(kernel=kernel, score=sec_b, inflight=sec_c)))


if __name__ == "__main__":
    main()
