"""What a verify step of prompt-lookup speculative decoding costs (Vidi1.5-9B decoder, random weights, the 60-minute caches of bench.py:
25 image + 10 audio keys per frame, random data) -> profiles/spec_decode.json.

  python tools/bench_spec.py [--frames 3600] [--rounds 3] [--steps 6] [--out profiles/spec_decode.json]

Measured per round, the arms alternating inside one process: the plain Lq = 1 decode step, and the verify step (k drafts + the last token,
one text_forward of k + 1 rows, the argmax of all rows, ONE device-to-host copy of the ids, the accept rule, the cache roll-back) at
k in {1, 3, 7, 15} (T2T of the k + 1 rows: vidi_rope_cache + vidi_attn_text), the drafts forced: all right (a replay of a recorded greedy run) and all wrong.  Times are device events around whole loops that end in a synchronise, every
shape warmed first; the spread is (max - min) / mean of a measurement over the rounds, the largest one is recorded.  Derived: the
BREAK-EVEN number of accepted drafts per verify step, (t_verify(k) - t_plain) / t_plain — a verify step yields 1 + accepted tokens, a plain
step 1 — and tokens/s if every draft were accepted.  The acceptance rate of a real checkpoint is NOT measured here (random weights emit noise)."""
import argparse
import dataclasses
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KS = (1, 3, 7, 15)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3600)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6, help="verify steps per measurement")
    ap.add_argument("--plain-steps", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "spec_decode.json"))
    a = ap.parse_args()
    from vidi_amd import config as C
    from vidi_amd import spec
    from vidi_amd.engine import VidiEngine
    from vidi_amd.weights import init_random_weights
    if not torch.cuda.is_available():
        raise SystemExit("bench_spec needs the GPU: a CPU run says nothing about a step's time")
    dt = torch.bfloat16
    cfg = dataclasses.replace(C.vidi15_9b(), vis_num_layers=1, aud_num_layers=1)        # the towers are not part of a decode step
    eng = VidiEngine(cfg, init_random_weights(cfg, seed=3, dtype=dt, device="cuda"), dtype=dt, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(5)
    n_img, n_aud = 25 * a.frames, 10 * a.frames
    img = (torch.randn((n_img, cfg.hidden_size), generator=g, device="cuda") * cfg.mm_std * eng.normalizer).to(dt)
    aud = (torch.randn((n_aud, cfg.hidden_size), generator=g, device="cuda") * cfg.mm_std * eng.normalizer).to(dt)
    mm = eng.mm_stream_prefill(img, None, aud, None, pre_normalized=True, check_masks=False)
    mm.img_any_valid = mm.aud_any_valid = True
    del img, aud
    L = 39
    ids = torch.randint(0, cfg.vocab_size, (1, L), generator=g, device="cuda")
    n_rec = (max(KS) + 1) * a.steps + 2

    def prefill(room):
        ts = eng.new_text_state(1, L + room + 2)
        hn = eng.text_forward(eng.embed_tokens(ids), torch.arange(L, device="cuda"), ts, mm, Lq=L)
        ts.n_valid = torch.tensor([L], device="cuda")
        _, nxt = eng.logits_argmax(hn.view(1, L, -1)[:, -1])
        torch.cuda.synchronize()
        return ts, nxt

    def plain(n):
        """n ordinary decode steps -> (ms per step, the greedy tokens: the first from the prefill)"""
        ts, nxt = prefill(n)
        toks = [int(nxt[0])]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            posn = ts.n_valid.clone(); ts.n_valid += 1
            hn = eng.text_forward(eng.embed_tokens(nxt), posn, ts, mm, Lq=1)
            _, nxt = eng.logits_argmax(hn)
            toks.append(int(nxt[0]))                                       # the per-step D2H sync of the greedy loop
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n, toks

    def verify(k, right, rec):
        """a.steps verify steps with k forced drafts -> (ms per step, accepted drafts per step)"""
        ts, _ = prefill(n_rec)
        at, accepted = 0, 0                                                # rec[at]: the last decided token, not in the cache yet
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            draft = rec[at + 1: at + 1 + k] if right else [(t + 1) % cfg.vocab_size for t in rec[at + 1: at + 1 + k]]
            p0 = ts.past_len
            step = torch.tensor([rec[at]] + draft, dtype=torch.int64, device="cuda")
            posn = ts.n_valid[0] + torch.arange(k + 1, dtype=torch.int64, device="cuda")
            ts.n_valid += k + 1
            hn = eng.text_forward(eng.embed_tokens(step), posn, ts, mm, Lq=k + 1)
            _, idx = eng.logits_argmax(hn)
            n_acc, _ = spec.accept_run(idx.tolist(), draft, (), 1 << 30)   # one D2H of the k + 1 ids
            eng.truncate_text_state(ts, p0 + n_acc + 1)
            accepted += n_acc
            at += n_acc + 1                                                # (the recorded run goes on as the context, whatever the argmax said)
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps, accepted / a.steps

    _, rec = plain(n_rec)                                                  # warm-up of the plain shapes + the recorded greedy run
    meas = {"plain": []}
    acc = {}
    for r in range(a.rounds + 1):                                          # round 0 warms every shape of both arms and is dropped
        ms, _ = plain(a.plain_steps)
        if r:
            meas["plain"].append(ms)
        for k in KS:
            for right in (True, False):
                key = f"k={k} {'accepted' if right else 'rejected'}"
                ms, per = verify(k, right, rec)
                if r:
                    meas.setdefault(key, []).append(ms)
                    acc[key] = per
    stat = lambda v: dict(ms=round(sum(v) / len(v), 3), min=round(min(v), 3), max=round(max(v), 3))      # noqa: E731
    spread = max((max(v) - min(v)) / (sum(v) / len(v)) for v in meas.values())
    t_plain = sum(meas["plain"]) / len(meas["plain"])
    mean = lambda key: sum(meas[key]) / len(meas[key])                                                    # noqa: E731
    table = []
    for k in KS:
        t_acc, t_rej = mean(f"k={k} accepted"), mean(f"k={k} rejected")
        table.append(dict(k=k, rows=k + 1, ms_all_accepted=round(t_acc, 3), ms_all_rejected=round(t_rej, 3),
                          accepted_per_step_in_the_replay=round(acc[f"k={k} accepted"], 2),
                          break_even_accepted_per_step=round((t_acc - t_plain) / t_plain, 3),
                          tokens_per_s_at_full_acceptance=round((k + 1) / t_acc * 1e3, 1)))
    out = dict(what="verify step of prompt-lookup speculative decoding against the plain decode step; see tools/bench_spec.py",
               device=torch.cuda.get_device_name(0), preset="vidi15_9b (random weights)", dtype="bf16", frames=a.frames, image_keys=n_img, audio_keys=n_aud,
               prompt_len=L, rounds=a.rounds, verify_steps_per_measurement=a.steps, plain_steps_per_measurement=a.plain_steps,
               plain_step=stat(meas["plain"]), plain_tokens_per_s=round(1e3 / t_plain, 1), largest_run_to_run_spread=round(spread, 4),
               table=table,
               acceptance_with_real_weights="not measured (no checkpoint reachable; random weights emit noise)",
               measurements={k: stat(v) for k, v in meas.items()})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("plain_step", "largest_run_to_run_spread", "table")}))


if __name__ == "__main__":
    main()
