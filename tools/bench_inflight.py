"""Many questions against ONE encoded video: successive static batches (`generate()`, what a caller could do before) against in-flight
batching (`generate_inflight()`) -> profiles/inflight_queries.json.

  python tools/bench_inflight.py [--frames 3600] [--rounds 3] [--prompts 64] [--out profiles/inflight_queries.json]

One process, one resident state: the Vidi1.5-9B decoder with random weights, bf16, the 60-minute caches of bench.py (25 image + 10 audio keys
per frame, random data).  Workload: 64 copies of one 39-token prompt whose last 4 tokens vary; every prompt's `max_new_tokens` is drawn once
from a seeded list in 8..128 (stored in the output); EOS is disabled (an id outside the vocabulary), so both arms produce the same token counts.
  arm A   generate() on 16 prompts at a time, in input order, each call with its batch's largest max_new_tokens (rows that are done emit pads)
  arm B   generate_inflight(max_rows = engine.max_inflight_rows()) with min_admit in {1, 2, 4}
The arms alternate inside a round; a warm-up round is dropped; device events around whole runs that end in a synchronise.  Per arm: wall time,
decode steps and mean live rows per step (counted on the engine's calls), useful tokens/s (the sum of the requested lengths over the wall time);
the step-count MODEL (arm A: the sum over batches of the largest length; arm B: vidi_amd.inflight.simulate_steps on the lengths); the
run-to-run spread (max - min) / mean, the largest over the arms."""
import argparse
import dataclasses
import json
import os
import random
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MIN_ADMITS = (1, 2, 4)
BATCH = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3600)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--prompts", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "inflight_queries.json"))
    a = ap.parse_args()
    from vidi_amd import config as C
    from vidi_amd.engine import VidiEngine
    from vidi_amd.inflight import simulate_steps, static_batch_steps
    from vidi_amd.model import VidiForCausalLM
    from vidi_amd.weights import init_random_weights
    if not torch.cuda.is_available():
        raise SystemExit("bench_inflight needs the GPU: a CPU run says nothing about a step's time")
    dt = torch.bfloat16
    cfg = dataclasses.replace(C.vidi15_9b(), vis_num_layers=1, aud_num_layers=1)        # the towers are not part of a decode step
    eng = VidiEngine(cfg, init_random_weights(cfg, seed=3, dtype=dt, device="cuda"), dtype=dt, device="cuda")
    model = VidiForCausalLM(cfg, {}, dtype=dt, device="cuda", engine=eng)
    g = torch.Generator(device="cuda").manual_seed(5)
    n_img, n_aud = 25 * a.frames, 10 * a.frames
    img = (torch.randn((n_img, cfg.hidden_size), generator=g, device="cuda") * cfg.mm_std * eng.normalizer).to(dt)
    aud = (torch.randn((n_aud, cfg.hidden_size), generator=g, device="cuda") * cfg.mm_std * eng.normalizer).to(dt)
    mm = eng.mm_stream_prefill(img, None, aud, None, pre_normalized=True, check_masks=False)
    mm.img_any_valid = mm.aud_any_valid = True
    del img, aud
    L, N = 39, a.prompts
    rng = random.Random(11)
    lengths = [rng.randint(8, 128) for _ in range(N)]
    base = torch.randint(0, cfg.vocab_size, (L,), generator=g, device="cuda").cpu()
    prompts = base.repeat(N, 1)
    prompts[:, -4:] = torch.randint(0, cfg.vocab_size, (N, 4), generator=torch.Generator().manual_seed(7))
    no_eos = cfg.vocab_size + 7
    rows = eng.max_inflight_rows()

    count = dict(steps=0, rows=0, prefills=0)
    tf, sp, sd = eng.text_forward, eng.slots_prefill, eng.slots_decode

    def text_forward(hidden, positions, ts, mm_, Lq, **kw):
        if kw.get("rows") is None:                                 # arm A (arm B's steps are counted on slots_decode; its prefills on slots_prefill)
            if Lq == 1:
                count["steps"] += 1; count["rows"] += ts.B
            elif not count.get("inside"):
                count["prefills"] += 1
        return tf(hidden, positions, ts, mm_, Lq, **kw)

    def slots_prefill(*args):
        count["prefills"] += 1
        count["inside"] = True
        try:
            return sp(*args)
        finally:
            count["inside"] = False

    def slots_decode(tslots, slot_ids, token_ids, mm_):
        count["steps"] += 1; count["rows"] += len(slot_ids)
        return sd(tslots, slot_ids, token_ids, mm_)
    eng.text_forward, eng.slots_prefill, eng.slots_decode = text_forward, slots_prefill, slots_decode

    def arm_a():
        n = 0
        for i in range(0, N, BATCH):
            out = model.generate(prompts[i: i + BATCH], mm_state=mm, max_new_tokens=max(lengths[i: i + BATCH]), eos_token_id=no_eos)
            n += int(out.shape[1])
        return n

    def arm_b(min_admit):
        outs = model.generate_inflight(list(prompts), mm_state=mm, max_new_tokens=lengths, eos_token_id=no_eos, min_admit=min_admit)
        assert [len(o) for o in outs] == lengths
        return sum(lengths)

    def timed(fn):
        count.update(steps=0, rows=0, prefills=0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1), dict(count)

    arms = [("A: generate() x 16", arm_a)] + [(f"B: in-flight, min_admit={m}", (lambda m=m: arm_b(m))) for m in MIN_ADMITS]
    meas, counted = {}, {}
    for r in range(a.rounds + 1):                                          # round 0 warms every shape of both arms and is dropped
        for name, fn in arms:
            ms, cnt = timed(fn)
            if r:
                meas.setdefault(name, []).append(ms)
                counted[name] = cnt
    useful = sum(lengths)
    model_steps = {arms[0][0]: static_batch_steps(lengths, BATCH)}
    for m in MIN_ADMITS:
        model_steps[f"B: in-flight, min_admit={m}"] = simulate_steps(lengths, rows, m)
    table = []
    for name, _ in arms:
        v = meas[name]
        mean = sum(v) / len(v)
        c, (ms_, mr_, mp_) = counted[name], model_steps[name]
        table.append(dict(arm=name, wall_ms=round(mean, 1), min_ms=round(min(v), 1), max_ms=round(max(v), 1), spread=round((max(v) - min(v)) / mean, 4),
                          decode_steps=c["steps"], mean_live_rows_per_step=round(c["rows"] / max(c["steps"], 1), 2), prefill_calls=c["prefills"],
                          useful_tokens_per_s=round(useful / mean * 1e3, 1),
                          model=dict(decode_steps=ms_, mean_rows_per_step=round(mr_ / max(ms_, 1), 2), prefill_calls=mp_)))
    t_a = table[0]["wall_ms"]
    for row in table[1:]:
        row["speedup_over_A_measured"] = round(t_a / row["wall_ms"], 3)
        row["speedup_over_A_step_model"] = round(table[0]["model"]["decode_steps"] / row["model"]["decode_steps"], 3)
    out = dict(what="many queries on one resident video: static batches of 16 against in-flight batching; see tools/bench_inflight.py",
               device=torch.cuda.get_device_name(0), preset="vidi15_9b (random weights)", dtype="bf16", frames=a.frames, image_keys=n_img, audio_keys=n_aud,
               prompt_len=L, prompts=N, max_rows=rows, rounds=a.rounds, max_new_tokens=lengths, useful_tokens=useful,
               largest_run_to_run_spread=max(r_["spread"] for r_ in table), table=table)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(dict(largest_run_to_run_spread=out["largest_run_to_run_spread"], table=table)))


if __name__ == "__main__":
    main()
