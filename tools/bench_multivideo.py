#!/usr/bin/env python
"""A/B of the decode step for a batch of DIFFERENT videos: the batch path (one decode loop over all rows, segmented cross-attention) against
the row-by-row arm (one greedy loop per video: what VIDI_MULTI_VIDEO=0 runs), in ONE process, arms alternated, device-synchronised.

    python tools/bench_multivideo.py [--videos 8 --frames 60] [--reps 5] [--out profiles/multivideo_batch.json]

Both arms decode against the SAME resident caches (`MMBatchState.videos[b]` is video b's one-video view of the batch's caches), so the
difference is the decode side alone: B x the weight stream and B x the launches, or once.  ms per decode step = (time of N + 1 greedy tokens
- time of 1) / N.  The byte model next to the measurement, from shapes: row by row B * W + sum_b KV_b, batched W + sum_b KV_b per generated
token (W: decoder weights + lm_head, KV_b: video b's cross-attention K/V over all layers)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


WHAT = ("tools/bench_multivideo.py on one MI355X: ms per decode step for a batch of different videos, the batch path against the row-by-row arm "
        "(one greedy loop per video on the same resident caches: the decode path VIDI_MULTI_VIDEO=0 and the parent commit run), one process, arms "
        "alternated, device-synchronised; byte model from shapes next to it")


def append_record(path, rec):
    """profiles/multivideo_batch.json: {"what": ..., "records": [...], + whatever else the file holds}; the record is appended"""
    doc = {"what": WHAT, "records": []}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc.setdefault("records", []).append(rec)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="vidi15_9b")
    ap.add_argument("--videos", type=int, default=8)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--prompt-len", type=int, default=39)
    ap.add_argument("--decode-steps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--out", default=None, help="append the record to the `records` of this JSON file (the shape of profiles/multivideo_batch.json)")
    a = ap.parse_args()
    from vidi_amd import config as C
    from vidi_amd.model import VidiForCausalLM
    from vidi_amd.weights import init_random_weights
    dev = "cuda:0"
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    cfg = getattr(C, a.preset)()
    model = VidiForCausalLM(cfg, init_random_weights(cfg, seed=3, dtype=dtype, device=dev), dtype=dtype, device=dev)
    eng = model.engine
    B, T = a.videos, a.frames
    S = cfg.vis_image_size
    Cw = -(-T // 30)                                           # 1 fps: 30-s Whisper windows
    g = torch.Generator(device=dev).manual_seed(5)
    images = [(torch.randn((T, 3, S, S), generator=g, device=dev) * 0.5).clamp_(-1, 1).to(dtype) for _ in range(B)]
    audios = [(torch.randn((Cw, cfg.aud_num_mel_bins, cfg.aud_nb_max_frames), generator=g, device=dev) * 0.3).to(dtype) for _ in range(B)]
    sizes = [T * 100] * B
    gi = torch.Generator().manual_seed(2)
    ids = torch.randint(1000, min(200000, cfg.vocab_size), (B, a.prompt_len + 1), generator=gi)
    ids[:, 0] = cfg.bos_token_id
    ids[:, 4] = -200

    # ---- does the batch's K/V fit?  (host integers, before anything is allocated) ----
    from vidi_amd.shard import audio_token_counts, image_tokens_per_frame
    nkv, hd, L = cfg.num_key_value_heads, cfg.head_dim, cfg.num_hidden_layers
    n_img = T * image_tokens_per_frame(cfg, B * T)
    n_aud = audio_token_counts(sizes[0], cfg)[1]
    r64 = lambda x: (x + 63) // 64 * 64                                           # noqa: E731
    kv_alloc = B * (r64(n_img) + r64(n_aud)) * L * 2 * nkv * hd * 2
    free, _ = torch.cuda.mem_get_info()
    rec = dict(preset=a.preset, videos=B, frames=T, prompt_len=a.prompt_len, decode_steps=a.decode_steps, dtype=a.dtype,
               keys_per_video=dict(image=n_img, audio=n_aud), kv_cache_bytes=kv_alloc, free_bytes_before=free)
    if kv_alloc * 1.25 > free:
        rec["skipped"] = "the K/V caches of the batch do not fit next to the weights"
        print(json.dumps(rec))
        return
    st = model.encode_mm_batch(images, audios, sizes)
    del images, audios
    torch.cuda.synchronize()

    N = a.decode_steps
    kw = dict(eos_token_id=10 ** 9, do_sample=False)

    def arm_batch(n):
        return model.generate(ids, mm_state=st, max_new_tokens=n, **kw)

    def arm_rows(n):
        return torch.cat([model.generate(ids[b: b + 1], mm_state=st.videos[b], max_new_tokens=n, **kw) for b in range(B)])

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    outs = {}
    for name, fn in (("batch", arm_batch), ("rows", arm_rows)):     # warm every shape of both arms
        for n in (1, N + 1):
            outs[name] = timed(fn, n)[1]
    same = float((outs["batch"] == outs["rows"]).float().mean())
    steps = {"batch": [], "rows": []}
    for _ in range(a.reps):
        for name, fn in (("rows", arm_rows), ("batch", arm_batch)):
            t1 = timed(fn, 1)[0]
            tn = timed(fn, N + 1)[0]
            steps[name].append((tn - t1) / N)
    wbytes = sum(t.numel() * t.element_size() for Ld in eng.layers for k, t in Ld.items() if k not in ("wkv", "wo_kv")) \
        + eng.lm_head.numel() * eng.lm_head.element_size()
    kv = [(v.n_img + v.n_aud) * L * 2 * nkv * hd * 2 for v in st.videos]
    model_rows, model_batch = B * wbytes + sum(kv), wbytes + sum(kv)
    summ = {k: dict(ms_per_step_median=statistics.median(v), min=min(v), max=max(v), all=[round(x, 3) for x in v]) for k, v in steps.items()}
    spread = max(summ["batch"]["max"] - summ["batch"]["min"], summ["rows"]["max"] - summ["rows"]["min"])
    rec.update(ms_per_decode_step=summ, spread_ms=spread, speedup=summ["rows"]["ms_per_step_median"] / summ["batch"]["ms_per_step_median"],
               gate_batch_shorter_by_more_than_spread=summ["rows"]["min"] - summ["batch"]["max"] > spread,
               tokens_equal_fraction=same,
               byte_model=dict(weights=wbytes, kv_per_video=kv[0], rows=model_rows, batch=model_batch, ratio=model_rows / model_batch))
    print(json.dumps(rec))
    if a.out:
        append_record(a.out, rec)
    if not rec["gate_batch_shorter_by_more_than_spread"]:
        sys.exit("the batch path's decode step is not shorter than the row-by-row arm's by more than the spread: a defect to explain")


if __name__ == "__main__":
    main()
