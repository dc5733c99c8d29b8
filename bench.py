#!/usr/bin/env python
"""bench.py — BASELINE.json's metric on MI355X: video-tokens/s of the Vidi1.5-9B prefill on a synthetic
1-hour video at 1 fps (3600 frames, 120 audio windows, 39-token temporal-retrieval prompt), plus s/query.

A "step" = one full prefill of the hot path with inputs already resident in HBM:
    SigLIP tower -> pool/projector/pos/norm -> Whisper tower -> audio pool/projector ->
    42-layer multimodal (diagonal) stream + cross-attention cache fill ->
    text prefill (T2T + T2V + T2A) -> first-token logits + argmax.
video-tokens/s = Nv * K / t   (Nv = 90 000 visual tokens at 3600 frames: the reference's token-budget rule).

N > 1 (torchrun, one rank per GPU): the SAME video is sharded along the frame axis (and 30-s audio
windows); every rank runs towers + stream on its shard, keeps its K/V shard resident and the per-layer
cross-attention partials are all-gathered (RCCL) and LSE-merged — strong scaling of one query.

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the K steps and prints the headline (`value`,
`ms_per_step`, stage times, the first-token logit digest); `--dump-outputs DIR` also saves what the last timed step computed.
`--full` adds the legs that take runs of their own, after the timed steps: roofline (dominant kernel family = MFMA GEMM, timed
with HIP events on the launch stream), decode / s-per-query, verify, the other BASELINE configs and dtype, box_reference,
preproc and cpu_baseline (the CPU oracle timed on a bounded slice of this workload).
"""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_PEAK_TFLOPS = 2500.0      # dense bf16/fp16, MI355X_MICROARCH.md
# The first-token ARGMAX of a random-init model with tied embeddings is decided by the prompt's last token (67480 in every record of
# rounds 1-3), whatever the video: masking every video key moves the first-token logits by 5 sigma yet leaves the argmax (measured at
# q_proj gains 1, 2 and 4: profiles/r4_notes.md).  What shows that the timed kernels computed the right thing is therefore not the token
# but the `verify` leg below; the gain option stays for experiments (FLOPs, bytes and shapes do not depend on it).
ATTN_GAIN = 1.0
# Bounds of the in-run verification.  Token embeddings are compared FREE-RUNNING (26 SigLIP / 32 Whisper layers + projector of bf16
# rounding noise between two bf16 evaluations): max |err| <= 0.12 of the spread (measured 0.045-0.081, profiles/r4_notes.md).  The decoder's
# diagonal stream is compared TEACHER-FORCED, layer by layer, on the rows the kernels saw (VidiEngine.probe): one layer's roundings,
# |err| <= atol x spread + rtol x |ref| — the bounds of tests/test_gpu_full_depth.py.
VERIFY_BOUND_EMBEDS = 0.12
VERIFY_KV_TOL = (1e-2, 1.2e-2)
VERIFY_STREAM_TOL = (4e-2, 2.5e-2)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=3600, help="video frames; 3600 @1 fps = BASELINE 60-min config")
    ap.add_argument("--fps", type=float, default=1.0, help="sampling rate of the frames: the video lasts frames / fps seconds, which sizes the "
                                                           "30-s audio windows and the mel length (BASELINE configs[4]: 3600 frames @2 fps = 30 min)")
    ap.add_argument("--prompt-len", type=int, default=39)
    ap.add_argument("--ragged-prompts", type=int, nargs=2, default=None, metavar=("MIN", "MAX"),
                    help="--queries prompts of lengths MIN..MAX (evenly spread, right-padded with an attention mask) instead of equal "
                         "lengths (SURVEY 8d config 5: 24 52)")
    ap.add_argument("--decode-steps", type=int, default=32)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-kernel-timer", action="store_true")
    ap.add_argument("--queries", type=int, default=1, help="prompts batched against the one encoded video (BASELINE config 5: 8)")
    ap.add_argument("--decode-graph", action="store_true", help="replay decode steps from a hipGraph (opt-in: capture costs ~126 ms)")
    ap.add_argument("--preset", default="vidi15_9b")
    ap.add_argument("--dist-mode", default=os.environ.get("VIDI_DIST_MODE", "sharded_stream"), choices=["sharded_stream", "gather_tokens"],
                    help="N > 1: 'sharded_stream' keeps every rank's tokens local through the decoder (K/V shards + per-layer LSE-merged cross-attention, "
                         "scales the whole prefill); 'gather_tokens' is BASELINE configs[3] as worded: frame-sharded towers + RCCL all-gather of the "
                         "visual / audio tokens, decoder replicated (scales the towers only)")
    ap.add_argument("--vis-chunk", type=int, default=0, help="override cfg.vis_frames_per_chunk (activation chunking only)")
    ap.add_argument("--aud-chunk", type=int, default=0, help="override cfg.aud_chunks_per_batch")
    ap.add_argument("--no-preproc", action="store_true", help="skip the extra (untimed-in-`value`) GPU preprocessing leg")
    ap.add_argument("--src-hw", type=int, nargs=2, default=[480, 854], help="decoded frame size fed to the preprocessing leg")
    ap.add_argument("--no-verify", action="store_true", help="skip the (untimed) oracle check of sampled frames / K/V-cache rows after the timed region")
    ap.add_argument("--no-other-dtype", action="store_true", help="skip the (untimed-in-`value`) leg that runs the headline workload once in the other 16-bit dtype")
    ap.add_argument("--no-other-configs", action="store_true", help="skip the (untimed-in-`value`) legs that run BASELINE configs[1] and configs[4] on this GPU "
                    "after the headline workload (default workload, one GPU only)")
    ap.add_argument("--attn-gain", type=float, default=ATTN_GAIN, help="factor on the decoder's random q_proj weights (a power of two is exact in "
                                                                        "bf16/fp16): sharper text->video attention; 1 = SURVEY 8d's plain randn * 0.02")
    ap.add_argument("--full", action="store_true", help="after the timed steps, also run every leg beside the headline: the instrumented pass "
                    "(kernel_families, roofline), the decode leg (s/query), verify, the other BASELINE configs and dtype, box_reference, preproc and "
                    "cpu_baseline (each --no-* option above switches its leg off again).  Without it a run times the K prefill steps and nothing else")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed to DIR/<name>.npy (float32; "
                                                                          "first-token logits and tokens in full, fixed samples of the token embeddings and K/V caches)")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if not a.full:              # a plain run is the headline alone
        a.no_kernel_timer = a.no_verify = a.no_other_configs = a.no_other_dtype = a.no_preproc = a.no_cpu_baseline = True
    return a


def self_launch(a):
    """`python bench.py --gpus N` outside torchrun: re-executes itself as N ranks (one per GPU) under torch.distributed.run and relays
    rank 0's JSON line.  Under torchrun (WORLD_SIZE set) this is never reached.  Test mode: VIDI_DIST_BACKEND=gloo lets the N ranks
    share GPU 0 of a one-GPU box (RCCL refuses two ranks on one device)."""
    import socket
    import subprocess
    ngpu = torch.cuda.device_count()
    env = dict(os.environ)
    if ngpu < a.gpus:
        if env.get("VIDI_DIST_BACKEND") != "gloo":
            raise SystemExit(f"bench.py --gpus {a.gpus}: only {ngpu} GPU(s) visible (set VIDI_DIST_BACKEND=gloo to run the ranks on one GPU as a test)")
        env.setdefault("VIDI_FORCE_DEVICE", "0")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC: what RCCL needs between the ranks' processes on this driver
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    # rank 0's JSON line is relayed alone: transports (gloo) print connection chatter on the ranks' stdout
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            print(line)
        elif line.strip():
            print(line, file=sys.stderr)
    raise SystemExit(r.returncode)


from vidi_amd.shard import shard          # noqa: E402  (the product's frame / window partition; host integer logic)


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _physical_cores():
    try:
        seen = set()
        phys = core = None
        for line in open("/proc/cpuinfo"):
            if line.startswith("physical id"):
                phys = line.split(":")[1].strip()
            elif line.startswith("core id"):
                core = line.split(":")[1].strip()
            elif not line.strip():
                if phys is not None and core is not None:
                    seen.add((phys, core))
                phys = core = None
        return len(seen) or None
    except OSError:
        return None


def cpu_baseline(cfg, T, Nv, Na, prompt_len, quick=False, windows=None):
    """The reference has no CPU path (FA2 is hard-required), so the baseline is the CPU oracle (oracle/vidi_oracle.py, eager
    PyTorch) on the host cores, timed on the slices SURVEY 8(d) prescribes and extrapolated linearly in (frames x layers),
    (tokens x layers), (windows x layers):  SigLIP 32 frames x 2 layers, LLM mm-stream 4 096 tokens x 2 layers, text->mm cross-attention
    of the prompt over ALL Nv keys x 2 layer-modality calls, Whisper 2 windows x 2 layers — in fp32 and bf16.  The thread count is swept
    on a GEMM probe of the stream's gate/up shape and the best one is used for every leg."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import dataclasses
    import vidi_oracle as O
    from vidi_amd.weights import init_random_weights
    cores = os.cpu_count() or 1
    nf, ntok, nwin, vis_l, llm_l, aud_l, x_calls = (4, 512, 1, 1, 1, 1, 1) if quick else (32, 4096, 2, 2, 2, 2, 2)
    # ---- thread sweep on one GEMM of the dominant shape (tokens x H) . (H x 2I) ----
    g = torch.Generator().manual_seed(0)
    a = torch.randn((ntok, cfg.hidden_size), generator=g)
    b = torch.randn((cfg.hidden_size, 2 * cfg.intermediate_size if not quick else 1024), generator=g)
    probe = {}
    cands = sorted({c for c in (8, 16, 32, 64, 128, 256, cores) if c <= cores})
    for dt in (torch.float32, torch.bfloat16):
        aa, bb = a.to(dt), b.to(dt)
        for n in cands:
            torch.set_num_threads(n)
            torch.matmul(aa, bb)
            t0 = time.perf_counter(); torch.matmul(aa, bb); dtm = time.perf_counter() - t0
            probe[(str(dt).split(".")[-1], n)] = 2.0 * aa.shape[0] * aa.shape[1] * bb.shape[1] / dtm / 1e12
    del a, b
    small = dataclasses.replace(cfg, num_hidden_layers=max(1, llm_l), vis_num_layers=vis_l + 1, aud_num_layers=aud_l, vocab_size=1024)
    w32 = init_random_weights(small, seed=3, dtype=torch.float32, device="cpu")
    names = {f.name for f in dataclasses.fields(O.OracleConfig)}
    ocfg = O.OracleConfig(**{k: v for k, v in small.to_dict().items() if k in names}, vis_select_layer=small.mm_vision_select_layer)
    C = math.ceil(T / 30) if windows is None else windows
    # algorithmic FLOPs of the slices (SURVEY 8d per-unit figures)
    Hv, Iv, Ns = cfg.vis_hidden_size, cfg.vis_intermediate_size, cfg.vis_side ** 2
    f_vis = (8 * Hv * Hv + 4 * Hv * Iv + 4 * Ns * Hv) * Ns                       # per frame-layer
    f_llm = 4 * cfg.hidden_size * 2 * cfg.num_key_value_heads * cfg.head_dim / 2 * 2 + 2 * cfg.num_attention_heads * cfg.head_dim * cfg.hidden_size \
        + 6 * cfg.hidden_size * cfg.intermediate_size                             # per token-layer (K,V proj + o_proj(V) + GeGLU MLP)
    Da, Fa, Nw = cfg.aud_d_model, cfg.aud_ffn_dim, cfg.aud_max_source_positions
    f_aud = (8 * Da * Da + 4 * Da * Fa + 4 * Nw * Da) * Nw                        # per window-layer
    f_x = 4.0 * prompt_len * cfg.num_attention_heads * cfg.head_dim               # per key per layer-modality call
    legs = {}
    for dt in (torch.float32, torch.bfloat16):
        name = str(dt).split(".")[-1]
        # every leg is timed at the three thread counts the GEMM probe ranks best for this dtype; the fastest time per leg is kept
        # (the towers' many small eager ops prefer fewer threads than the big stream GEMMs)
        thr = sorted(cands, key=lambda n: -probe[(name, n)])[:3] if not quick else cands[-1:]
        w = w32 if dt == torch.float32 else {k: (v.to(dt) if v.is_floating_point() else v) for k, v in w32.items()}
        g = torch.Generator().manual_seed(0)
        px = ((torch.randn((nf, 3, cfg.vis_image_size, cfg.vis_image_size), generator=g) * 0.5).clamp(-1, 1)).to(dt)
        x = (torch.randn((1, ntok, cfg.hidden_size), generator=g) * 0.03 * cfg.hidden_size ** 0.5).to(dt)
        mel = (torch.randn((nwin, cfg.aud_num_mel_bins, cfg.aud_nb_max_frames), generator=g) * 0.3).to(dt)
        # cross attention of the text prefill over ALL video keys (GQA-expanded like repeat_kv, gemma.py:74-75)
        nk = Nv if not quick else 4096
        q = torch.randn((1, cfg.num_attention_heads, prompt_len, cfg.head_dim), generator=g).to(dt)
        k = torch.randn((1, cfg.num_attention_heads, nk, cfg.head_dim), generator=g).to(dt)

        def leg_siglip():
            O.siglip_forward(px, w, ocfg)

        def leg_llm():
            for li in range(llm_l):
                O.mm_stream_layer(x, w, f"model.layers.{li}.", ocfg)

        def leg_aud():
            O.whisper_encoder_forward(mel, w, ocfg)

        def leg_x():
            for _ in range(x_calls):
                O.sdpa_reference(q, k, k, cfg.head_dim ** -0.5, 50.0)

        best_t, best_n = {}, {}
        with torch.no_grad():
            torch.set_num_threads(thr[0])
            O.siglip_forward(px[:1], w, ocfg)                                     # first-touch / allocator warm-up
            for n in thr:
                torch.set_num_threads(n)
                for lname, fn in (("siglip", leg_siglip), ("llm_stream", leg_llm), ("whisper", leg_aud), ("xattn", leg_x)):
                    t0 = time.perf_counter(); fn(); tl = time.perf_counter() - t0
                    if lname not in best_t or tl < best_t[lname]:
                        best_t[lname], best_n[lname] = tl, n
        del px, x, mel, q, k
        t_vis, t_llm = best_t["siglip"] / (nf * vis_l), best_t["llm_stream"] / (ntok * llm_l)
        t_aud, t_x = best_t["whisper"] / (nwin * aud_l), best_t["xattn"] / (nk * x_calls)
        nthr = best_n["llm_stream"]
        parts = {"siglip": T * cfg.vis_select_layers * t_vis, "llm_stream": (Nv + Na) * cfg.num_hidden_layers * t_llm,
                 "whisper": C * cfg.aud_num_layers * t_aud, "xattn": (Nv + Na) * cfg.num_hidden_layers * t_x}
        t_total = sum(parts.values())
        legs[name] = {"value": Nv / t_total, "threads": nthr, "threads_per_leg": best_n, "t_prefill_extrapolated_s": t_total, "breakdown_s": parts,
                      "cpu_tflops": {"gemm_probe": probe[(name, thr[0])], "siglip": f_vis / t_vis / 1e12, "llm_stream": f_llm / t_llm / 1e12,
                                     "whisper": f_aud / t_aud / 1e12, "xattn": f_x / t_x / 1e12},
                      "effective_tflops": (T * cfg.vis_select_layers * f_vis + (Nv + Na) * cfg.num_hidden_layers * f_llm +
                                           C * cfg.aud_num_layers * f_aud + (Nv + Na) * cfg.num_hidden_layers * f_x) / t_total / 1e12}
    best = max(legs, key=lambda n: legs[n]["value"])
    # `cores` (the contract's key) = `threads_used` = the threads the winning leg actually ran on (the sweep picks them per leg);
    # `host_threads` / `host_cores_physical` = what the box offers
    return {"value": legs[best]["value"], "unit": "video-tokens/s", "cores": legs[best]["threads"], "threads_used": legs[best]["threads"],
            "host_threads": cores, "host_cores_physical": _physical_cores(), "kind": "port",
            "dtype": best, "cpu_model": _cpu_model(),
            "sample": f"oracle (eager PyTorch, fp32 and bf16; the faster one is `value`) on {nf} frames x {vis_l} SigLIP layers, {ntok} tokens x "
                      f"{llm_l} LLM stream layers, {nwin} Whisper windows x {aud_l} layers, x-attn Lq={prompt_len} over {nk} keys x {x_calls} calls; "
                      f"extrapolated linearly to {T} frames / {Nv + Na} tokens / {C} windows / "
                      f"{cfg.vis_select_layers}+{cfg.num_hidden_layers}+{cfg.aud_num_layers} layers",
            "t_prefill_extrapolated_s": legs[best]["t_prefill_extrapolated_s"], "by_dtype": legs,
            "thread_sweep_gemm_tflops": {f"{d}@{n}": v for (d, n), v in probe.items()}}


def synth_normal(first: int, count: int, stream: int, dev) -> torch.Tensor:
    """`count` standard-normal fp32 values that depend only on (stream, global element index first .. first + count): splitmix64 of the
    index gives two 24-bit uniforms, Box-Muller turns them into one normal.  int64 arithmetic wraps (two's complement) on every device."""
    def s64(c):                                     # the constants of splitmix64 as signed 64-bit values
        return c - (1 << 64) if c >= (1 << 63) else c

    def lsr(x, n):                                  # logical shift right of an int64 tensor
        return (x >> n) & ((1 << (64 - n)) - 1)

    def mix(z):
        z = (z ^ lsr(z, 30)) * s64(0xBF58476D1CE4E5B9)
        z = (z ^ lsr(z, 27)) * s64(0x94D049BB133111EB)
        return z ^ lsr(z, 31)

    i = torch.arange(first, first + count, dtype=torch.int64, device=dev)
    z = mix((i * 2 + 0) * s64(0x9E3779B97F4A7C15) + stream)
    u1 = (lsr(z, 40).to(torch.float32) + 0.5) * (1.0 / (1 << 24))
    z = mix((i * 2 + 1) * s64(0x9E3779B97F4A7C15) + stream)
    u2 = (lsr(z, 40).to(torch.float32) + 0.5) * (1.0 / (1 << 24))
    del z, i
    return torch.sqrt(-2.0 * torch.log(u1)).mul_(torch.cos(u2.mul_(2.0 * math.pi)))


def _oracle_frame_embeds(O, px, t_global, T, w, ocfg, normalizer_dtype):
    """Token embeddings (inputs of the decoder's multimodal stream) of the frames `px` = frames `t_global` of a T-frame video:
    oracle/vidi_oracle.py:encode_video_images restricted to a few frames, with the GLOBAL frame count deciding the token budget and
    the GLOBAL index addressing pos_t (multimodal.py:156-208), then `* normalizer` (gemma.py:353-355)."""
    import torch
    m = "model."
    feats = O.siglip_forward(px, w, ocfg)
    side, pool, d = ocfg.vis_side, ocfg.mm_image_pool_size, ocfg.hidden_size
    feats = feats.reshape(len(feats), side, side, -1).permute(0, 3, 1, 2)
    if ocfg.arch == "mistral":
        feats = O.learned_conv2d_pool(feats, w[m + "mm_rand_img_pool.conv.weight"], pool)
    else:
        feats = O.conv2d_pool(feats, O.token_budget_hw(T, side, pool, ocfg.mm_max_tokens_base), pool)
    feats = feats.permute(0, 2, 3, 1)
    feats = O.projector_mlp(feats, w, m + "mm_rand_img_projector.")
    feats = O.mm_RMSNorm(feats, w[m + "mm_rand_img_norm.weight"])
    ph = O.learnable_pos_embd(feats.shape[1], pool, d, w, m + "mm_rand_pos_h.", feats.dtype)
    feats = feats + O.mm_rms_norm(ph.reshape(1, -1, 1, d))
    pw = O.learnable_pos_embd(feats.shape[2], pool, d, w, m + "mm_rand_pos_w.", feats.dtype)
    feats = feats + O.mm_rms_norm(pw.reshape(1, 1, -1, d))
    pt = O.learnable_pos_embd(T, ocfg.mm_time_interval, d, w, m + "mm_rand_pos_t.", feats.dtype)
    feats = feats + O.mm_rms_norm(pt[torch.as_tensor(t_global)].reshape(-1, 1, 1, d))
    feats = feats.flatten(1, 2)
    mask = torch.sum(torch.abs(feats), dim=-1) != 0
    feats = O.mm_RMSNorm(feats, w[m + "mm_rand_llm_norm.weight"]) * mask.unsqueeze(-1)
    if ocfg.arch != "mistral":
        feats = feats * torch.tensor(d ** 0.5, dtype=normalizer_dtype)
    return feats


def _oracle_window_embeds(O, mel, c_global, audio_size, w, ocfg, normalizer_dtype):
    """The same for whole 30-s audio windows `c_global` (windows that the global floors of multimodal.py:226-235 do not clip)."""
    import torch
    import torch.nn.functional as F
    m = "model."
    feats = O.whisper_encoder_forward(mel, w, ocfg)                                  # [n, 1500, Da]
    pool, d = ocfg.mm_audio_pool_size, ocfg.hidden_size
    s2_total = O.audio_token_counts([audio_size], ocfg)[1][0]
    per = feats.shape[1] // pool
    x = F.conv1d(feats.permute(0, 2, 1), w[m + "mm_rand_aud_pool.weight"], None, stride=pool).permute(0, 2, 1)      # [n, per, .]
    x = O.projector_mlp(x, w, m + "mm_rand_aud_projector.")
    x = O.mm_RMSNorm(x, w[m + "mm_rand_aud_norm.weight"])
    pt = O.learnable_pos_embd(s2_total, ocfg.mm_time_interval, d, w, m + "mm_rand_pos_t.", x.dtype)
    rows = torch.stack([torch.arange(c * per, (c + 1) * per) for c in c_global])
    x = x + O.mm_rms_norm(pt[rows])
    mask = torch.sum(torch.abs(x), dim=-1) != 0
    x = O.mm_RMSNorm(x, w[m + "mm_rand_llm_norm.weight"]) * mask.unsqueeze(-1)
    if ocfg.arch != "mistral":
        x = x * torch.tensor(d ** 0.5, dtype=normalizer_dtype)
    return x


def _cache_rows(mm, li, rows, nkv, hd):
    """K and V rows `rows` (local key indices) of layer li out of the tiled caches -> two [n, nkv*hd] fp32 host tensors"""
    r = torch.as_tensor(rows, dtype=torch.int64, device=mm.kc.device)
    k = mm.kc[li].reshape(nkv, -1, hd)[:, r].permute(1, 0, 2).reshape(len(rows), nkv * hd)
    tk = r & 31
    x = tk & 15
    pos = (tk & ~15) | (8 * ((x >> 2) & 1) + (x & 3) + 4 * (x >> 3))                # perm16 key order inside a 32-key sub-tile
    v = mm.vtc[li][:, r >> 5, :, pos]                                               # [n, nkv, hd]
    return k.float().cpu(), v.reshape(len(rows), nkv * hd).float().cpu()


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, logits, tokens, fi, fa, mm, nkv, hd):
    """`--dump-outputs DIR`: what the last timed step handed its caller, as float32 .npy files, so that two builds can be compared output
    for output on the same seeded inputs.  In full: the first-token logits [queries, vocab] and their argmax.  Sampled (fixed seed, so the
    same rows every run): 256 rows of the video token embeddings, 128 of the audio token embeddings, and the K / V cache rows of 256 video
    and 128 audio keys at the first and the last decoder layer.  Under N ranks these are rank 0's local rows."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    rs = np.random.RandomState(0)

    def pick(n, k):
        return np.sort(rs.choice(n, min(n, k), replace=False)) if n > 0 else np.zeros(0, dtype=np.int64)

    def rows(x, k):
        if x is None or x.shape[0] == 0:
            return np.zeros((0, 0), dtype=np.float32)
        return x[torch.as_tensor(pick(x.shape[0], k), device=x.device)].float().cpu().numpy()

    keys = np.concatenate([mm.img_start + pick(mm.n_img, 256), mm.aud_start + pick(mm.n_aud, 128)]).tolist()
    kv = [_cache_rows(mm, li, keys, nkv, hd) for li in (0, mm.kc.shape[0] - 1)] if keys else []
    out = {"first_token_logits": logits.float().cpu().numpy(), "first_token": tokens.cpu().numpy().astype(np.float32),
           "video_tokens_sample": rows(fi, 256), "audio_tokens_sample": rows(fa, 128),
           "k_cache_sample": np.stack([k.numpy() for k, _ in kv]) if kv else np.zeros((0, 0, 0), dtype=np.float32),
           "v_cache_sample": np.stack([v.numpy() for _, v in kv]) if kv else np.zeros((0, 0, 0), dtype=np.float32)}
    total = sum(x.nbytes for x in out.values())
    if total > DUMP_LIMIT_BYTES:
        raise RuntimeError(f"bench: --dump-outputs would write {total / 2**20:.1f} MB, more than {DUMP_LIMIT_BYTES >> 20} MB")
    for name, x in out.items():
        np.save(os.path.join(out_dir, name + ".npy"), x)


def verify_against_oracle(a, cfg, eng, model, make_weights, dtype, dev, world, rank, pixel, mel, f0, f1, T, c0, c1, audio_size, Nv, Na,
                          fi, fa, mi_mask, ma_mask, mm, idt, mask, pos, lg0, ff0=None, fc0=None):
    """Untimed check of what the timed kernels produced, against the CPU oracle (oracle/vidi_oracle.py — the checker, never the thing
    measured) evaluated in the model dtype with the reference's eager rounding points:
      * FREE-RUNNING: the token embeddings of three frames (first / middle / last: SigLIP x26 -> pool -> projector -> norms -> positions)
        and of one 30-s audio window (Whisper x32 -> Conv1d pool -> projector -> norm -> positions), as the timed step produced them;
      * TEACHER-FORCED, every decoder layer: one more pass of the diagonal stream with the engine's probe keeping 64 sampled rows (image
        + audio keys; first / last rows, frame edges, random rows) of the residual stream at every layer's input.  The stream is
        row-wise, so the oracle evaluates each layer on exactly those rows and must reproduce that layer's K / V cache rows and the
        next layer's input within one layer's bf16 roundings — and the probed pass must equal the timed pass's caches bit for bit;
      * how much the first-token logits move when every video key is masked (the multimodal path must matter to the answer).
    Every rank checks the sampled rows / frames it owns (global indices, so the sample is the same for every N); results are MAX-reduced.
    `ff0` / `fc0`: the frame / window that row 0 of `fi` / `fa` belongs to — this rank's first (sharded stream: its own tokens) or 0 (dist
    mode gather_tokens: after the all-gather every rank holds all tokens; the frames it can re-encode are still its own)."""
    ff0 = f0 if ff0 is None else ff0
    fc0 = c0 if fc0 is None else fc0
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import dataclasses
    import numpy as np
    import vidi_oracle as O
    t_begin = time.perf_counter()
    names = {f.name for f in dataclasses.fields(O.OracleConfig)}
    d = {k: v for k, v in cfg.to_dict().items() if k in names}
    d["vis_select_layer"] = cfg.mm_vision_select_layer
    d["arch"] = cfg.arch
    ocfg = O.OracleConfig(**d)
    nkv, hd, Lr = cfg.num_key_value_heads, cfg.head_dim, cfg.num_hidden_layers
    tpf = Nv // T
    per = cfg.aud_max_source_positions // cfg.mm_audio_pool_size
    spread = lambda got, ref: float((got.float() - ref.float()).abs().max() / ref.float().std())
    errs = {"embeds_frames": 0.0, "embeds_audio": 0.0, "kv": 0.0}
    counts = {"frames": 0, "windows": 0, "kv_rows": 0}
    per_layer = {}

    # the probed pass of the diagonal stream (part 2): every rank runs it at the same time (under shards mm_stream_prefill agrees on
    # global key counts); it keeps the sampled rows of the residual stream at every layer's input
    rs = np.random.RandomState(7)
    g_img = sorted(set([0, 1, tpf - 1, tpf, Nv // 2, Nv - 1] + rs.randint(0, Nv, 42).tolist()))
    g_aud = sorted(set([0, Na // 2, Na - 1] + rs.randint(0, Na, 13).tolist())) if Na > 0 else []
    img0, aud0 = ff0 * tpf, fc0 * per
    n_il, n_al = (0 if fi is None else fi.shape[0]), (0 if fa is None else fa.shape[0])
    li_rows = [r - img0 for r in g_img if img0 <= r < img0 + n_il]
    la_rows = [r - aud0 for r in g_aud if aud0 <= r < aud0 + n_al]
    keys = li_rows + [mm.aud_start + r for r in la_rows]
    eng.probe = {"stream_rows": torch.as_tensor(keys, dtype=torch.int64, device=dev), "stream_x": []}
    try:
        with torch.no_grad():
            mmv = eng.mm_stream_prefill(fi, mi_mask, fa, ma_mask, pre_normalized=True)
    finally:
        sx = [t.cpu() for t in eng.probe["stream_x"]]
        eng.probe = None

    def local_checks():
        """parts (1) and (2): rank-local (no collective inside)"""
        wdev = make_weights()                   # the original (not repacked) parameters again: same seed, same tensors

        class HostView:                         # tensors cross to the host when the oracle asks for them (one layer at a time)
            def __getitem__(self, k): return wdev[k].cpu()
            def __contains__(self, k): return k in wdev
            def get(self, k, default=None): return wdev[k].cpu() if k in wdev else default

        w = HostView()
        # ---- (1) token embeddings of sampled frames / one audio window ----
        mine = [t for t in sorted({0, T // 2, T - 1}) if f0 <= t < f1]
        if mine and fi is not None and fi.shape[0]:
            ref = _oracle_frame_embeds(O, pixel[[t - f0 for t in mine]].cpu(), mine, T, w, ocfg, dtype)
            got = torch.stack([fi[(t - ff0) * tpf: (t - ff0 + 1) * tpf] for t in mine]).cpu()
            errs["embeds_frames"] = spread(got, ref)
            counts["frames"] = len(mine)
        if c0 == 0 and c1 > 0 and fa is not None and fa.shape[0] >= per and Na >= per:
            ref = _oracle_window_embeds(O, mel[:1].cpu(), [0], audio_size, w, ocfg, dtype)
            errs["embeds_audio"] = spread(fa[:per].cpu()[None], ref)
            counts["windows"] = 1
        # ---- (2) the diagonal stream, teacher-forced: the oracle evaluates each layer on exactly the rows the probed pass kept ----
        if keys:
            use = lambda got, ref, tol: float(((got.float() - ref.float()).abs() / (tol[0] * float(ref.float().std()) + tol[1] * ref.float().abs())).max())
            for li in range(Lr):
                x_next, kref, vref = O.mm_stream_layer(sx[li][None], w, f"model.layers.{li}.", ocfg)
                kg, vg = _cache_rows(mmv, li, keys, nkv, hd)
                kg0, vg0 = _cache_rows(mm, li, keys, nkv, hd)
                if not (torch.equal(kg, kg0) and torch.equal(vg, vg0)):
                    per_layer[li] = float("inf")                   # the probed pass must reproduce the timed pass bit for bit
                    continue
                u = max(use(kg, kref[0], VERIFY_KV_TOL), use(vg, vref[0], VERIFY_KV_TOL))
                if li + 1 < Lr:
                    u = max(u, use(sx[li + 1], x_next[0], VERIFY_STREAM_TOL))
                per_layer[li] = u
                errs["kv_spread"] = max(errs.get("kv_spread", 0.0), spread(kg, kref[0]), spread(vg, vref[0]))
            errs["kv"] = max(per_layer.values())
            counts["kv_rows"] = len(keys)
        del wdev
        torch.cuda.empty_cache()

    shared_gpu = world > 1 and os.environ.get("VIDI_FORCE_DEVICE") is not None       # test mode: the ranks share one GPU's memory
    torch.set_num_threads(max(8, min(64, (os.cpu_count() or 8) // (1 if shared_gpu else world))))
    with torch.no_grad():
        if shared_gpu:
            import torch.distributed as dist
            for r in range(world):              # one rank at a time holds the second copy of the parameters
                if r == rank:
                    local_checks()
                dist.barrier()
        else:
            local_checks()
        mmv = None                      # frees the probed pass's caches
        # ---- (3) the answer must depend on the video: first-token logits with every image key masked ----
        mm_blind = dataclasses.replace(mm, img_mask=torch.zeros(max(64, (mm.n_img + 63) // 64 * 64), dtype=torch.uint8, device=dev), img_any_valid=False)
        _, last2 = model._prefill(idt, mask, pos, mm_blind, 1)
        lg2, tk2 = eng.logits_argmax(last2)
        shift = float((lg2.float() - lg0.float()).abs().max() / lg0.float().std())
        tk_seen = torch.argmax(lg0.float(), dim=-1)
        token_moves = bool((tk2.cpu() != tk_seen.cpu()).any())
    worst_layer = max(per_layer, key=per_layer.get) if per_layer else -1
    vals = [errs["embeds_frames"], errs["embeds_audio"], errs["kv"], errs.get("kv_spread", 0.0)]
    if world > 1:
        import torch.distributed as dist
        red_dev = "cpu" if dist.get_backend() == "gloo" else dev
        e = torch.tensor([v if math.isfinite(v) else 1e30 for v in vals], dtype=torch.float64, device=red_dev)
        c = torch.tensor([counts["frames"], counts["windows"], counts["kv_rows"]], dtype=torch.int64, device=red_dev)
        dist.all_reduce(e, op=dist.ReduceOp.MAX)
        dist.all_reduce(c, op=dist.ReduceOp.SUM)
        vals = e.tolist()
        counts = dict(zip(("frames", "windows", "kv_rows"), (int(x) for x in c.tolist())))
    ok = (vals[0] <= VERIFY_BOUND_EMBEDS and vals[1] <= VERIFY_BOUND_EMBEDS and vals[2] <= 1.0
          and counts["frames"] > 0 and counts["kv_rows"] > 0 and math.isfinite(shift))
    return {"ok": bool(ok), "oracle": f"oracle/vidi_oracle.py in {str(dtype).split('.')[-1]} with the reference's eager rounding points (CPU)",
            "embeds_frames_max_err": vals[0], "embeds_audio_max_err": vals[1], "embeds_bound": VERIFY_BOUND_EMBEDS,
            "embeds_unit": "free-running, max |got - ref| / std(ref)", "frames_checked": counts["frames"], "audio_windows_checked": counts["windows"],
            "kv_rows": counts["kv_rows"], "kv_layers_checked": Lr, "kv_tolerance_used": vals[2], "bound": 1.0,
            "kv_unit": "teacher-forced per layer, max |err| / (atol x std(ref) + rtol x |ref|); K / V rows with (atol, rtol) = %s, next-layer input rows with %s"
                       % (VERIFY_KV_TOL, VERIFY_STREAM_TOL),
            "kv_rows_max_err": vals[3], "kv_rows_max_err_unit": "max |got - ref| / std(ref) over the K / V rows of all layers",
            "kv_worst_layer_this_rank": worst_layer,
            "first_token_logit_shift_when_video_masked": shift, "first_token_changes_when_video_masked": token_moves,
            "seconds": time.perf_counter() - t_begin}


def main():
    a = parse()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(a)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != max(1, a.gpus) and int(os.environ.get("RANK", "0")) == 0:
        print(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world}: running {world} rank(s)", file=sys.stderr)
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    import torch.distributed as dist
    force_dev = os.environ.get("VIDI_FORCE_DEVICE")          # test hook: several ranks on one GPU (gloo transport)
    if force_dev is not None:
        local = int(force_dev)
    if world > 1:
        torch.cuda.set_device(local)
        dist.init_process_group(backend=os.environ.get("VIDI_DIST_BACKEND", "nccl"))
    dev = f"cuda:{local if (world > 1 or force_dev is not None) else 0}"
    torch.cuda.set_device(dev)
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16

    from vidi_amd import config as C, hip
    from vidi_amd.engine import token_budget_hw, audio_token_counts
    from vidi_amd.model import VidiForCausalLM
    from vidi_amd.weights import init_random_weights
    cfg = getattr(C, a.preset)()
    if a.vis_chunk > 0:
        cfg.vis_frames_per_chunk = a.vis_chunk
    if a.aud_chunk > 0:
        cfg.aud_chunks_per_batch = a.aud_chunk
    def make_weights():
        w = init_random_weights(cfg, seed=3, dtype=dtype, device=dev)            # replicated on every rank (same seed)
        if a.attn_gain != 1.0:
            for li in range(cfg.num_hidden_layers):
                w[f"model.layers.{li}.self_attn.q_proj.weight"] *= a.attn_gain
        return w

    weights = make_weights()
    model = VidiForCausalLM(cfg, weights, dtype=dtype, device=dev)
    del weights
    eng = model.engine
    if world > 1:
        eng.set_dist(None, mode=a.dist_mode)
    gather_mode = world > 1 and a.dist_mode == "gather_tokens"

    # ---- synthetic workload: resident in HBM before the timed region ----
    T = a.frames
    secs = T / a.fps                                          # dataset/vid_utils.py:10-14 load_video(fps=...): T frames cover T / fps seconds
    Cw = math.ceil(secs / 30)                                 # 30-s Whisper windows
    audio_size = int(round(secs * 100))                       # mel frames (100 per second)
    f0, f1 = shard(T, world, rank)
    c0, c1 = shard(Cw, world, rank)
    from vidi_amd.shard import video_shard
    vshard = video_shard(T, Cw, world, rank)
    assert (vshard.f0, vshard.f1, vshard.c0, vshard.c1) == (f0, f1, c0, c1)
    # the synthetic video is a function of the GLOBAL element index (a counter-based generator: splitmix64 of the index -> two uniforms ->
    # Box-Muller), so an N-rank run encodes exactly the video the 1-rank run does and `first_token` / `verify` are comparable across N;
    # generated in chunks of 64 frames by a few large elementwise launches (one generator call per frame was 14 400 tiny launches, which
    # rocprofv3's counter mode did not survive)
    S = cfg.vis_image_size
    pixel = torch.empty((f1 - f0, 3, S, S), dtype=dtype, device=dev)
    per_frame = 3 * S * S
    for a0 in range(f0, f1, 64):
        a1 = min(f1, a0 + 64)
        pixel[a0 - f0: a1 - f0] = synth_normal(a0 * per_frame, (a1 - a0) * per_frame, 0x51A1, dev).mul_(0.5).clamp_(-1, 1).view(a1 - a0, 3, S, S).to(dtype)
    per_win = cfg.aud_num_mel_bins * cfg.aud_nb_max_frames
    mel = torch.empty((c1 - c0, cfg.aud_num_mel_bins, cfg.aud_nb_max_frames), dtype=dtype, device=dev)
    for a0 in range(c0, c1, 64):
        a1 = min(c1, a0 + 64)
        mel[a0 - c0: a1 - c0] = synth_normal(a0 * per_win, (a1 - a0) * per_win, 0xA0D1, dev).mul_(0.3).view(a1 - a0, cfg.aud_num_mel_bins, cfg.aud_nb_max_frames).to(dtype)
    gi = torch.Generator().manual_seed(2)
    plens = [a.prompt_len] * a.queries
    if a.ragged_prompts is not None:
        lo, hi = a.ragged_prompts
        plens = [lo + round(i * (hi - lo) / max(1, a.queries - 1)) for i in range(a.queries)]
    ids = torch.randint(1000, min(200000, cfg.vocab_size), (a.queries, max(plens) + 1), generator=gi)
    ids[:, 0] = cfg.bos_token_id
    ids[:, 4] = -200
    amask = None
    if len(set(plens)) > 1:                                    # right-padded batch (multimodal.py:413-432 re-pads on the right)
        amask = torch.arange(ids.shape[1])[None, :] < (torch.tensor(plens)[:, None] + 1)
        ids = torch.where(amask, ids, torch.full_like(ids, cfg.pad_token_id if cfg.pad_token_id is not None else 0))
    if cfg.arch == "mistral":                                   # Vidi-7B: fixed pool x pool tokens per frame (learned Conv2DPool)
        Nv = T * cfg.mm_image_pool_size ** 2
    else:
        hw = token_budget_hw(T, cfg.vis_side, cfg.mm_image_pool_size, cfg.mm_max_tokens_base)
        h, w = hw if hw[0] != 28 else (cfg.vis_side + 1, cfg.vis_side + 1)
        Nv = T * (h // cfg.mm_image_pool_size) * (w // cfg.mm_image_pool_size)
    Na = audio_token_counts(audio_size, cfg)[1]

    def whole_sample_flag(x):
        """the sample-level "any non-zero input" flag (`torch.sum(torch.abs(x)) != 0`, multimodal.py:202, 246), computed INSIDE the timed step as
        the reference does: one reduction over this rank's frames / windows (vidi_any_nonzero), OR-ed over the ranks when the sample is sharded"""
        flag = eng.sample_flag(x)
        if world > 1:
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        return flag

    from vidi_amd.model import strip_image_token
    idt, mask, pos = strip_image_token(ids, amask)
    stage_ms = {}
    checks = []            # (first-token logits, argmax) of every timed step: verified after the timed region (finite, identical)
    last_feats = [None] * 4     # the last step's video / audio token embeddings + masks (inputs of the stream): the verify leg reads sampled rows

    def ev():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def step(record=False):
        e0 = ev()
        fi, mi = eng.encode_video_images(pixel, frame_offset=f0, total_frames=T, normalizer=eng.normalizer, sample_flag=whole_sample_flag(pixel))
        e1 = ev()
        fa, ma = eng.encode_video_audios(mel, audio_size, normalizer=eng.normalizer, chunk_offset=c0, sample_flag=whole_sample_flag(mel))
        e2 = ev()
        if gather_mode:      # the all-gather of visual / audio tokens (the product's own helper: model.encode_mm_state calls the same)
            fi, mi, fa, ma = model._gather_tokens(fi, mi, fa, ma, vshard, audio_size)
        e2b = ev()
        mm = eng.mm_stream_prefill(fi, mi, fa, ma, pre_normalized=True)
        e3 = ev()
        ts, last = model._prefill(idt, mask, pos, mm, a.decode_steps + 1)
        logits, nxt = eng.logits_argmax(last)
        e4 = ev()
        checks.append((logits, nxt))
        last_feats[:] = [fi, fa, mi, ma]
        if record:
            torch.cuda.synchronize()
            for k, (x, y) in {"vision_encode": (e0, e1), "audio_encode": (e1, e2), "token_all_gather": (e2, e2b), "mm_stream": (e2b, e3), "text_prefill": (e3, e4)}.items():
                stage_ms[k] = stage_ms.get(k, 0.0) + x.elapsed_time(y)
        return mm, ts, nxt

    def barrier():
        if world > 1:
            dist.barrier()

    def decode_eager(ts, mm, nxt, n):
        for _ in range(n):
            emb = eng.embed_tokens(nxt)
            posn = ts.n_valid.clone(); ts.n_valid += 1
            hn = eng.text_forward(emb, posn, ts, mm, Lq=1)
            _, nxt = eng.logits_argmax(hn)
            int(nxt[0])                                       # per-token D2H sync, as a stopping criterion needs
        return nxt

    for _ in range(a.warmup):
        wmm, wts, wnxt = step()
        if a.full:
            decode_eager(wts, wmm, wnxt, min(2, a.decode_steps))   # warm the decode leg's kernels too (code objects, workspaces)
        del wmm, wts, wnxt
    # ---- timed region: K steps with NO per-launch instrumentation (the headline number) ----
    checks.clear()
    barrier(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        mm, ts, nxt = step(record=True)
    torch.cuda.synchronize(); barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    ms_per_step = dt / a.steps * 1e3
    value = Nv * a.steps / dt
    # every timed step must have produced finite first-token logits and THE SAME BITS (same inputs, deterministic kernels: no atomics in any
    # reduction, fixed split-K orders).  The argmax alone would let a sporadic ring / `vmcnt` race through that perturbs a few logits without
    # flipping the token; the full [queries, vocab] logit rows are compared bit for bit, and their SHA-256 goes into the line.
    import hashlib
    lg0, tk0 = checks[0]
    if not bool(torch.isfinite(lg0.float()).all()):
        raise RuntimeError("bench: non-finite first-token logits in a timed step")
    differing = [i for i, (lg, tk) in enumerate(checks) if not (torch.equal(lg, lg0) and torch.equal(tk, tk0))]
    if differing:
        worst = max(float((checks[i][0].float() - lg0.float()).abs().max()) for i in differing)
        raise RuntimeError(f"bench: first-token logits of timed step(s) {differing} differ bitwise from step 0 (max |diff| {worst:.3g}): "
                           "a run-to-run race in a kernel of the prefill")
    first_token = [int(x) for x in tk0.tolist()]
    logit_checksum = float(lg0.float().abs().sum())
    logits_sha256 = hashlib.sha256(lg0.contiguous().view(torch.int16).cpu().numpy().tobytes()).hexdigest()
    n_bitwise = len(checks)
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, checks[-1][0], checks[-1][1], last_feats[0], last_feats[1], mm, cfg.num_key_value_heads, cfg.head_dim)
    checks.clear()

    # ---- second pass (untimed in `value`): every C-ABI launch bracketed with HIP events on the launch stream -> kernel families ----
    timer = None if a.no_kernel_timer else hip.KernelTimer()
    timer_steps = 0
    if timer is not None:
        timer_steps = min(a.steps, 2)
        saved = dict(stage_ms)
        barrier(); torch.cuda.synchronize()
        hip.TIMER = timer
        for _ in range(timer_steps):
            mm, ts, nxt = step()
        torch.cuda.synchronize(); barrier()
        hip.TIMER = None
        stage_ms.clear(); stage_ms.update(saved)
        if not all(torch.equal(lg, lg0) and torch.equal(tk, tk0) for lg, tk in checks):
            raise RuntimeError("bench: the instrumented pass's first-token logits differ bitwise from the timed pass")
        n_bitwise += len(checks)
        checks.clear()

    # ---- decode leg (s/query = prefill + n_new decode steps on the resident caches) ----
    # --decode-graph: the step is captured once in a hipGraph (vidi_amd/engine.py:make_decode_graph) and replayed;
    # the capture (one eager step + graph build) is timed inside the leg, so s/query pays for it.
    # over shards the captured step includes the per-layer RCCL all-gathers (engine.make_decode_graph); the gloo test transport cannot be captured
    use_graph = a.decode_graph and a.decode_steps >= 2 and (world == 1 or dist.get_backend() == "nccl")
    t_capture = 0.0
    if a.full:
        torch.cuda.synchronize()
        td0 = time.perf_counter()
        if use_graph:
            nxt, replay = eng.make_decode_graph(ts, mm, nxt)
            int(nxt[0])
            t_capture = time.perf_counter() - td0
            for _ in range(a.decode_steps - 1):
                nxt = replay(nxt)
                int(nxt[0])                                       # per-token D2H sync, as a stopping criterion needs
        else:
            nxt = decode_eager(ts, mm, nxt, a.decode_steps)
        torch.cuda.synchronize()
        t_total_decode = time.perf_counter() - td0
        t_decode = t_total_decode / max(1, a.decode_steps)
        t_replay = (t_total_decode - t_capture) / max(1, a.decode_steps - 1) if use_graph else t_decode

    # ---- verification leg (untimed): sampled frames' token embeddings and sampled K/V-cache rows against the CPU oracle ----
    verify = None
    if not a.no_verify:
        verify = verify_against_oracle(a, cfg, eng, model, make_weights, dtype, dev, world, rank, pixel, mel, f0, f1, T, c0, c1, audio_size, Nv, Na,
                                       last_feats[0], last_feats[1], last_feats[2], last_feats[3], mm, idt, mask, pos, lg0,
                                       ff0=0 if gather_mode else None, fc0=0 if gather_mode else None)
        if not verify["ok"]:
            if rank == 0:
                print(json.dumps({"verify": verify}), file=sys.stderr)
            raise RuntimeError("bench: the HIP path disagrees with the oracle on the sampled rows (see `verify` on stderr)")

    # ---- the other single-GPU BASELINE configurations, measured in the same run (never part of `value`) ----
    # configs[1]: 5-min video @1 fps, one query; configs[4] on ONE GPU: 30 min @2 fps (3 600 frames), 8 ragged prompts sharing the video, 128
    # decoded tokens per query.  Same synthetic video (its first frames / windows), same weights, one warm-up + one timed prefill each.
    other = None
    if world == 1 and not a.no_other_configs and a.preset == "vidi15_9b" and a.frames == 3600 and a.fps == 1.0 and a.queries == 1:
        del mm, ts
        torch.cuda.empty_cache()

        def run_config(T2, fps2, queries2, ragged2, ndec, eng=eng, model=model, pixel=pixel, mel=mel):
            secs2 = T2 / fps2
            Cw2, asz2 = math.ceil(secs2 / 30), int(round(secs2 * 100))
            px2, mel2 = pixel[:T2], mel[:Cw2]

            def decode_eager(ts, mm, nxt, n):
                for _ in range(n):
                    emb = eng.embed_tokens(nxt)
                    posn = ts.n_valid.clone(); ts.n_valid += 1
                    hn = eng.text_forward(emb, posn, ts, mm, Lq=1)
                    _, nxt = eng.logits_argmax(hn)
                    int(nxt[0])
                return nxt
            pl2 = [a.prompt_len] * queries2 if ragged2 is None else [ragged2[0] + round(i * (ragged2[1] - ragged2[0]) / max(1, queries2 - 1)) for i in range(queries2)]
            g2 = torch.Generator().manual_seed(2)
            ids2 = torch.randint(1000, min(200000, cfg.vocab_size), (queries2, max(pl2) + 1), generator=g2)
            ids2[:, 0] = cfg.bos_token_id
            ids2[:, 4] = -200
            am2 = None
            if len(set(pl2)) > 1:
                am2 = torch.arange(ids2.shape[1])[None, :] < (torch.tensor(pl2)[:, None] + 1)
                ids2 = torch.where(am2, ids2, torch.full_like(ids2, cfg.pad_token_id if cfg.pad_token_id is not None else 0))
            idt2, mask2, pos2 = strip_image_token(ids2, am2)
            hw2 = token_budget_hw(T2, cfg.vis_side, cfg.mm_image_pool_size, cfg.mm_max_tokens_base)
            h2, w2 = hw2 if hw2[0] != 28 else (cfg.vis_side + 1, cfg.vis_side + 1)
            Nv2 = T2 * (h2 // cfg.mm_image_pool_size) * (w2 // cfg.mm_image_pool_size)
            Na2 = audio_token_counts(asz2, cfg)[1]

            def prefill():
                e = [ev()]
                fi, mi = eng.encode_video_images(px2, frame_offset=0, total_frames=T2, normalizer=eng.normalizer, sample_flag=eng.sample_flag(px2)); e.append(ev())
                fa, ma = eng.encode_video_audios(mel2, asz2, normalizer=eng.normalizer, chunk_offset=0, sample_flag=eng.sample_flag(mel2)); e.append(ev())
                mm2 = eng.mm_stream_prefill(fi, mi, fa, ma, pre_normalized=True); e.append(ev())
                ts2, last2 = model._prefill(idt2, mask2, pos2, mm2, ndec + 1)
                _, nx2 = eng.logits_argmax(last2); e.append(ev())
                return mm2, ts2, nx2, e
            w = prefill()
            decode_eager(w[1], w[0], w[2], 2)
            del w
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mm2, ts2, nx2, e = prefill()
            torch.cuda.synchronize()
            t_pre = time.perf_counter() - t0
            td = time.perf_counter()
            nx2 = decode_eager(ts2, mm2, nx2, ndec)
            torch.cuda.synchronize()
            t_dec = (time.perf_counter() - td) / max(1, ndec)
            if not bool(torch.isfinite(nx2.float()).all()):
                raise RuntimeError("non-finite decode output")
            rec = {"frames": T2, "fps": fps2, "queries": queries2, "prompt_tokens": pl2 if len(set(pl2)) > 1 else pl2[0], "video_tokens": Nv2, "audio_tokens": Na2,
                   "video_tokens_per_s": Nv2 / t_pre, "prefill_ms": t_pre * 1e3, "decode_ms_per_step": t_dec * 1e3, "decode_tokens": ndec,
                   "sec_per_query": (t_pre + ndec * t_dec) / queries2,
                   "stage_ms": dict(zip(("vision_encode", "audio_encode", "mm_stream", "text_prefill"), (e[i].elapsed_time(e[i + 1]) for i in range(4))))}
            del mm2, ts2
            torch.cuda.empty_cache()
            return rec
        try:
            other = {"configs[1] 5-min@1fps, 1 query": run_config(300, 1.0, 1, None, a.decode_steps),
                     "configs[4] on ONE GPU: 30-min@2fps, 8 ragged prompts, 128 tokens": run_config(3600, 2.0, 8, (24, 52), 128),
                     "note": "same run, same box, after the timed headline steps; one warm-up + one timed prefill each; never part of `value`"}
        except Exception as e:          # never lose the headline line to an extra leg
            other = {"error": repr(e)}
        # the headline workload once more in the OTHER 16-bit dtype (the reference's inference dtype is fp16: builder.py:41, eval/inference.py:23;
        # BASELINE quotes bf16): a second engine with the same seed's weights, one warm-up + one timed prefill + the decode steps
        if other is not None and "error" not in other and not a.no_other_dtype:
            try:
                odt_name = "fp16" if a.dtype == "bf16" else "bf16"
                odt = torch.float16 if odt_name == "fp16" else torch.bfloat16
                model2 = VidiForCausalLM(cfg, init_random_weights(cfg, seed=3, dtype=odt, device=dev), dtype=odt, device=dev)
                rec = run_config(T, a.fps, a.queries, a.ragged_prompts, a.decode_steps, eng=model2.engine, model=model2, pixel=pixel.to(odt), mel=mel.to(odt))
                rec["dtype"] = odt_name
                rec["relative_to_headline_dtype"] = rec["video_tokens_per_s"] / value
                other[f"configs[2] headline workload in {odt_name} (one timed prefill)"] = rec
                del model2
                torch.cuda.empty_cache()
            except Exception as e:
                other[f"headline workload in the other dtype"] = {"error": repr(e)}

    # ---- box-speed reference (untimed): frozen probe kernels, so that records from different boxes can be normalised ----
    box = None
    if a.full:
        try:
            box = hip.probe_box(pixel)
        except Exception as e:
            box = {"error": repr(e)}

    fam = timer.summary() if timer is not None else {}
    roof = None
    if "gemm" in fam:
        gm = fam["gemm"]
        ach = gm["work"] / (gm["ms"] * 1e-3) / 1e12
        roof = {"kernel": "gemm_w4_kernel / gemm_kernel (MFMA 16x16x32, 256x256x64 tiles, persistent 4-wave; all GEMM launches of the instrumented steps)",
                "bound": "mfma", "achieved": ach, "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": ach / MFMA_PEAK_TFLOPS, "traffic": None,
                "launches": gm["launches"], "avg_launch_ms": gm["ms"] / gm["launches"],
                "algorithmic_flop_per_launch_avg": gm["work"] / gm["launches"],
                "algorithmic_bytes_per_launch_avg": gm["bytes"] / gm["launches"]}
        # L2-miss bytes per launch come from separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over this same command
        # (tools/traffic_from_pmc.py -> profiles/); PMC passes cannot run inside the timed region.  The committed summary is attached
        # ONLY when it was taken on this exact GEMM source (digest of the kernel sources + flags), workload and launch mix.
        from vidi_amd.build import source_digest
        dig = source_digest("gemm")
        roof["gemm_source_digest"] = dig
        tpath = os.path.join(ROOT, "profiles", "traffic.json")
        roof["traffic_note"] = "no PMC summary for this build (profiles/traffic.json absent)"
        if os.path.exists(tpath) and world == 1:
            tj = json.load(open(tpath))
            if tj.get("gemm_source_digest") != dig:
                roof["traffic_note"] = f"profiles/traffic.json was collected on GEMM source {tj.get('gemm_source_digest')}, not this build: not attached"
            elif tj.get("frames") != T or tj.get("launches_fetch_pass") != gm["launches"] // max(1, timer_steps) or tj.get("preset") != a.preset:
                roof["traffic_note"] = "profiles/traffic.json was collected on another workload / launch mix: not attached"
            else:
                roof["traffic"] = tj["hbm_bytes_per_launch"]
                roof["traffic_note"] = ("rocprofv3 --pmc FETCH_SIZE (x2, gfx950 correction) + WRITE_SIZE per GEMM launch, " + tj.get("file", "profiles/traffic.json") +
                                        "; the counters sit at the L2's fabric side, so Infinity-Cache hits are included: an upper bound on HBM bytes")
    fams = {k: {"launches": v["launches"], "ms_per_step": v["ms"] / max(1, timer_steps),
                ("TFLOP/s" if v["unit"] == "flop" else "GB/s"): (v["work"] / (v["ms"] * 1e-3) / (1e12 if v["unit"] == "flop" else 1e9)) if v["ms"] > 0 else 0.0}
            for k, v in fam.items()}

    res = {
        "metric": f"video-tokens/sec (prefill), Vidi1.5-9B {'1h' if secs == 3600 else f'{secs / 60:g}min'}@{a.fps:g}fps" if cfg.arch != "mistral" else "video-tokens/sec (prefill), Vidi-7B", "value": value, "unit": "video-tokens/s",
        "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": ms_per_step, "higher_is_better": True,
        "scaling": "strong", "vs_baseline": None, "dtype": a.dtype, "data": "synthetic (random frames/mel/prompt, random-init weights)",
        "config": {"workload": f"{'Vidi-7B' if cfg.arch == 'mistral' else 'Vidi1.5-9B'} prefill, {T} frames@{a.fps:g}fps 384px (+{Cw} audio windows, "
                               + (f"{a.prompt_len}-token prompt)" if len(set(plens)) == 1 and a.queries == 1 else f"{a.queries} prompts of {min(plens)}..{max(plens)} tokens sharing the video)"),
                   "frames": T, "fps": a.fps, "video_tokens": Nv, "audio_tokens": Na, "prompt_tokens": plens[0] if len(set(plens)) == 1 else plens,
                   "parallelism": ("single GPU" if world == 1 else f"frame-shard x{world} (towers sharded, RCCL all-gather of visual / audio tokens, decoder replicated)"
                                   if gather_mode else f"frame-shard x{world} (K/V shards resident, LSE-merged cross-attention)")},
        "dist_mode": a.dist_mode if world > 1 else None, "queries": a.queries, "frames_per_s": T * a.steps / dt,
        "stage_ms_per_step": {k: v / a.steps for k, v in stage_ms.items()},
        "first_token": first_token, "first_token_logit_abs_sum": logit_checksum,
        "first_token_logits_sha256": logits_sha256, "steps_with_bitwise_identical_first_token_logits": n_bitwise, "attn_gain": a.attn_gain,
    }
    if a.full:
        res.update({
            # one video, `queries` prompts answered together: the encode + stream prefill is shared
            "sec_per_query": (ms_per_step / 1e3 + a.decode_steps * t_decode) / a.queries, "decode_ms_per_token": t_decode * 1e3,
            "sec_per_query_cached": (stage_ms.get("text_prefill", 0.0) / a.steps / 1e3 + a.decode_steps * t_decode) / a.queries,
            "decode_tokens": a.decode_steps, "decode_graph": bool(use_graph), "decode_graph_capture_ms": t_capture * 1e3,
            "decode_replay_ms_per_token": t_replay * 1e3, "verify": verify, "kernel_families": fams, "kernel_family_steps": timer_steps,
            "roofline": roof, "box_reference": box, "other_baseline_configs": other,
        })
    if world == 1 and not a.no_preproc:
        # SURVEY §8f-2 leg, reported beside the metric and never part of `value`: decoded RGB frames (uint8) and 16 kHz PCM
        # resident in HBM -> pixel_values / input_features through csrc/preproc.hip (bit-exact with PIL + the HF processors)
        try:
            from vidi_amd.preproc import FramePreprocessor, LogMelExtractor
            H0, W0 = a.src_hw
            gp = torch.Generator(device=dev).manual_seed(7)
            frames_u8 = torch.randint(0, 256, (T, H0, W0, 3), dtype=torch.uint8, device=dev, generator=gp)
            pcm = torch.randn(int(round(secs * 16000)), device=dev, generator=gp) * 0.1
            fp = FramePreprocessor(cfg.vis_image_size, dtype=dtype, device=dev, frames_per_chunk=512)
            lm = LogMelExtractor(n_mels=cfg.aud_num_mel_bins, dtype=dtype, device=dev)
            fp(frames_u8[:8]); lm(pcm[: 480000 * 2]); torch.cuda.synchronize()
            tp0 = time.perf_counter()
            px2 = fp(frames_u8)
            mel2, alen = lm(pcm)
            torch.cuda.synchronize()
            t_pre = time.perf_counter() - tp0
            assert px2.shape == pixel.shape and mel2.shape == mel.shape and alen == audio_size
            res["preproc"] = {"ms_per_video": t_pre * 1e3, "source": f"{T} frames {H0}x{W0} RGB uint8 + {secs:g} s PCM, resident in HBM",
                              "value_incl_preproc": Nv / (ms_per_step / 1e3 + t_pre)}
            del frames_u8, pcm, px2, mel2
        except Exception as e:
            res["preproc"] = {"error": repr(e)}
    if rank == 0 and world == 1 and not a.no_cpu_baseline:
        try:
            res["cpu_baseline"] = cpu_baseline(cfg, T, Nv, Na, max(plens), windows=Cw)
            res["speedup_vs_cpu"] = value / res["cpu_baseline"]["value"]
        except Exception as e:      # never lose the GPU line to a host-side problem
            res["cpu_baseline"] = {"error": repr(e)}
    if rank == 0:
        print(json.dumps(res))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
