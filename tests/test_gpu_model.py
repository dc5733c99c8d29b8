"""Engine-level parity on the GPU: towers, encode pipeline, the D-Attn decoder and greedy generate
against the fp32 CPU oracle, on seeded synthetic weights (tiny config = every padding path; plus a
2-layer model with the real Gemma2-9B layer dims).  Tolerances: model dtype is bf16/fp16 with the
reference's rounding points, the oracle is fp32 => errors accumulate over layers; stated per test."""
import dataclasses

import pytest
import torch

import vidi_oracle as O
from util import logit_tol, report, seeded, unpack_vt, perm_positions

pytestmark = pytest.mark.gpu


def oracle_cfg(cfg) -> O.OracleConfig:
    names = {f.name for f in dataclasses.fields(O.OracleConfig)}
    d = {k: v for k, v in cfg.to_dict().items() if k in names}
    d["vis_select_layer"] = cfg.mm_vision_select_layer
    d["arch"] = cfg.arch
    return O.OracleConfig(**d)


def make(cfg, dtype, seed=3):
    from vidi_amd.weights import init_random_weights
    from vidi_amd.engine import VidiEngine
    w = init_random_weights(cfg, seed=seed, dtype=dtype, device="cpu")
    w32 = {k: v.float() for k, v in w.items()}
    eng = VidiEngine(cfg, dict(w), dtype=dtype, device="cuda", free_source=False)
    return eng, w32


@pytest.fixture(scope="module", params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def tiny_setup(request):
    from vidi_amd.config import tiny
    cfg = tiny()
    eng, w32 = make(cfg, request.param)
    return cfg, eng, w32, request.param


def tol(dt, k=1.0, tight=False):
    """activations after several bf16 layers: |err| <= 5% of the tensor's rms + 3% relative (fp16: 1% / 0.6%); tight (towers, encode
    pipelines, K/V caches, which use less than half of that — VIDI_TEST_REPORT audit): 3% + 2% (fp16: 0.6% / 0.4%)"""
    if tight:
        return (3e-2 * k, 2e-2) if dt == torch.bfloat16 else (6e-3 * k, 4e-3)
    return (5e-2 * k, 3e-2) if dt == torch.bfloat16 else (1e-2 * k, 6e-3)


def test_siglip_tower(tiny_setup):
    cfg, eng, w32, dt = tiny_setup
    T = 5                                                    # > vis_frames_per_chunk: exercises chunking
    px = seeded((T, 3, cfg.vis_image_size, cfg.vis_image_size), 100, 0.5).clamp(-1, 1).to(dt)
    ref = O.siglip_forward(px.float(), w32, oracle_cfg(cfg))
    got = eng.siglip_forward(px.cuda())
    report("siglip", got, ref, *tol(dt, ref.std().item(), tight=True))


def test_whisper_tower(tiny_setup):
    cfg, eng, w32, dt = tiny_setup
    C = 3
    mel = seeded((C, cfg.aud_num_mel_bins, cfg.aud_nb_max_frames), 101, 0.3).to(dt)
    ref = O.whisper_encoder_forward(mel.float(), w32, oracle_cfg(cfg))
    got = eng.whisper_forward(mel.cuda())
    report("whisper", got, ref, *tol(dt, ref.std().item(), tight=True))


@pytest.mark.parametrize("base", [60000, 50])
def test_encode_video_images(tiny_setup, base):
    """base=50 forces the token-budget resize branch (multimodal.py:175-180) at tiny size"""
    cfg, eng, w32, dt = tiny_setup
    cfg2 = dataclasses.replace(cfg, mm_max_tokens_base=base)
    eng.cfg = cfg2
    try:
        T = 4
        px = seeded((T, 3, cfg.vis_image_size, cfg.vis_image_size), 102, 0.5).clamp(-1, 1).to(dt)
        px[:, :, :3] = 0
        ocfg = oracle_cfg(cfg2)
        feats_ref, mask_ref = O.encode_video_images([px.float()], w32, ocfg)
        feats, mask = eng.encode_video_images(px.cuda())
        assert torch.equal(mask.cpu().bool(), mask_ref[0]), "token mask must be bit-exact"
        report("encode_video_images", feats, feats_ref[0], *tol(dt, feats_ref.std().item(), tight=True))
        # frame-axis sharding: two shards with global (offset,total) == the full encode, bit for bit
        vis = eng.siglip_forward(px.cuda())
        fa, ma = eng.encode_video_images(px[:2].cuda(), frame_offset=0, total_frames=T, vis_features=vis[:2])
        fb, mb = eng.encode_video_images(px[2:].cuda(), frame_offset=2, total_frames=T, vis_features=vis[2:])
        assert torch.equal(torch.cat([fa, fb]).cpu(), feats.cpu()), "frame shards must concatenate to the unsharded result"
    finally:
        eng.cfg = cfg


def test_encode_video_audios(tiny_setup):
    cfg, eng, w32, dt = tiny_setup
    C = 2
    mel = seeded((C, cfg.aud_num_mel_bins, cfg.aud_nb_max_frames), 103, 0.3).to(dt)
    audio_size = 173                                        # mel frames; floors: 86 -> 17 tokens
    feats_ref, mask_ref = O.encode_video_audios([mel.float()], [audio_size], w32, oracle_cfg(cfg))
    feats, mask = eng.encode_video_audios(mel.cuda(), audio_size)
    assert feats.shape[0] == feats_ref.shape[1] == 17
    assert torch.equal(mask.cpu().bool(), mask_ref[0])
    report("encode_video_audios", feats, feats_ref[0], *tol(dt, feats_ref.std().item(), tight=True))


def _run_oracle_prefill(w32, ocfg, ids, img, imask, aud, amask):
    idl, am, pos = O.strip_image_token(ids)
    emb = O.embed_text(idl, am, w32)
    caches = O.OracleCaches()
    hidden = O.model_forward(emb, pos, am, img, imask, aud, amask, w32, ocfg, caches, 0)
    return hidden, caches, am


def test_decoder_prefill_and_caches(tiny_setup):
    """D-Attn decoder: mm stream caches of every layer + text hidden states after prefill"""
    cfg, eng, w32, dt = tiny_setup
    ocfg = oracle_cfg(cfg)
    H = cfg.hidden_size
    Nv, Na = 70, 21                                          # not multiples of 32/64
    img = (seeded((1, Nv, H), 104, cfg.mm_std)).to(dt); aud = (seeded((1, Na, H), 105, cfg.mm_std)).to(dt)
    img[0, 7] = 0                                             # a masked token
    imask = torch.ones((1, Nv), dtype=torch.bool); imask[0, 7] = False
    amask = torch.ones((1, Na), dtype=torch.bool)
    ids = torch.tensor([[2, 11, 12, -200, 13, 14, 15, 16, 17]], dtype=torch.int64)
    href, caches, am = _run_oracle_prefill(w32, ocfg, ids, img.float(), imask, aud.float(), amask)

    from vidi_amd.model import strip_image_token
    mm = eng.mm_stream_prefill(img[0].cuda(), imask[0].to(torch.uint8).cuda(), aud[0].cuda(), amask[0].to(torch.uint8).cuda(),
                               pre_normalized=False)
    assert mm.img_mask is not None and mm.aud_mask is None
    nkv, hd = cfg.num_key_value_heads, cfg.head_dim
    for li in range(cfg.num_hidden_layers):
        kref, vref = caches.image[li]
        kc = mm.kc[li].reshape(nkv, -1, hd)[:, :Nv].permute(1, 0, 2).reshape(Nv, -1)
        report(f"image K cache L{li}", kc, kref[0], *tol(dt, kref.std().item(), tight=True))
        pos = torch.from_numpy(perm_positions(32))
        vt = mm.vtc[li].cpu()[:, :, :, pos]                   # undo perm16 inside each 32-key sub-tile
        v = vt.permute(1, 3, 0, 2).reshape(-1, nkv * hd)[:Nv]
        report(f"image V cache L{li}", v, vref[0], *tol(dt, vref.std().item(), tight=True))
        karef, _ = caches.audio[li]
        ka = mm.kc[li].reshape(nkv, -1, hd)[:, mm.aud_start: mm.aud_start + Na].permute(1, 0, 2).reshape(Na, -1)
        report(f"audio K cache L{li}", ka, karef[0], *tol(dt, karef.std().item(), tight=True))
    idt, mask, pos_ids = strip_image_token(ids)
    ts = eng.new_text_state(1, 16)
    emb = eng.embed_tokens(idt.cuda())
    hn = eng.text_forward(emb, pos_ids.reshape(-1).cuda(), ts, mm, Lq=idt.shape[1], new_mask=mask.cuda())
    report("text hidden (prefill)", hn, href[0], *tol(dt, href.std().item()))


def test_generate_matches_oracle(tiny_setup):
    """end-to-end: video + audio + prompt -> greedy tokens.  Token ids must equal the oracle's wherever
    the oracle's top-2 logit margin exceeds the numeric tolerance; prefill logits within tolerance."""
    cfg, eng, w32, dt = tiny_setup
    from vidi_amd.model import VidiForCausalLM
    ocfg = oracle_cfg(cfg)
    T, C = 3, 1
    px = seeded((T, 3, cfg.vis_image_size, cfg.vis_image_size), 106, 0.5).clamp(-1, 1).to(dt)
    mel = seeded((C, cfg.aud_num_mel_bins, cfg.aud_nb_max_frames), 107, 0.3).to(dt)
    ids = torch.tensor([[2, 21, 22, 23, -200, 24, 25, 26]], dtype=torch.int64)
    n_new = 6
    ref_ids, dbg = O.generate_greedy(ids, [px.float()], [mel.float()], [100], w32, ocfg, n_new, return_debug=True)
    model = VidiForCausalLM.__new__(VidiForCausalLM)
    model.config, model.dtype, model.device, model.engine = cfg, dt, torch.device("cuda"), eng
    from types import SimpleNamespace
    model.generation_config = SimpleNamespace(eos_token_id=cfg.eos_token_id, pad_token_id=0)
    model.model = None
    out = model.forward(ids, images=px[None].cuda(), audios=mel[None].cuda(), audio_sizes=[100], logits_to_keep=1)
    ref_logits = dbg["prefill_logits"]
    ltol = logit_tol(dt, ref_logits)
    report("prefill logits", out.logits[:, -1], ref_logits, ltol, 0.0)
    got = model.generate(ids, images=px[None].cuda(), audios=mel[None].cuda(), audio_sizes=[100], max_new_tokens=n_new,
                         do_sample=False, use_cache=True).cpu()
    # compare token by token until the first low-margin step
    top2 = torch.topk(ref_logits[0].float(), 2).values
    if float(top2[0] - top2[1]) > 2 * ltol:
        assert int(got[0, 0]) == int(ref_ids[0, 0]), f"first token {int(got[0,0])} != oracle {int(ref_ids[0,0])}"
    assert got.shape[1] <= n_new and got.dtype == torch.int64


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_text_longer_than_the_sliding_window(dt):
    """gemma.py:104 + TP gemma2 sliding layers (even layers: key j visible to query i iff i - W <= j <= i) with the text LONGER than the
    window — every other model-level test keeps prompt + generation inside it.  tiny config with a window of 4: a 14-token prompt (its
    later rows must not see the first tokens on the even layers) and 8 teacher-forced decode steps that push the window further along,
    against the oracle's logits at every step (the oracle's window rule is the one the reference-executed goldens pin for in-window text;
    flash-attn's window semantics themselves are restated)."""
    from vidi_amd.config import tiny
    from vidi_amd.model import strip_image_token
    cfg = tiny(sliding_window=4)
    eng, w32 = make(cfg, dt, seed=21)
    ocfg = oracle_cfg(cfg)
    px = seeded((2, 3, cfg.vis_image_size, cfg.vis_image_size), 130, 0.5).clamp(-1, 1).to(dt)
    mel = seeded((1, cfg.aud_num_mel_bins, cfg.aud_nb_max_frames), 131, 0.3).to(dt)
    ids = torch.tensor([[2, 21, 22, 23, -200, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33]], dtype=torch.int64)
    n_new = 8
    ref_ids, dbg = O.generate_greedy(ids, [px.float()], [mel.float()], [100], w32, ocfg, n_new + 1, return_debug=True)
    # the window must matter in the oracle itself, or this test checks nothing
    wide = O.generate_greedy(ids, [px.float()], [mel.float()], [100], w32, dataclasses.replace(ocfg, sliding_window=4096), 1, return_debug=True)[1]
    assert float((wide["prefill_logits"] - dbg["prefill_logits"]).abs().max()) > 1e-3 * float(dbg["prefill_logits"].std())
    fi, mi = eng.encode_video_images(px.cuda())
    fa, ma = eng.encode_video_audios(mel.cuda(), 100)
    mm = eng.mm_stream_prefill(fi, mi, fa, ma, pre_normalized=False)
    idt, mask, pos = strip_image_token(ids)
    L = idt.shape[1]
    ts = eng.new_text_state(1, L + n_new + 2)
    hn = eng.text_forward(eng.embed_tokens(idt.cuda()), pos.reshape(-1).cuda(), ts, mm, Lq=L, new_mask=mask.cuda())
    ts.n_valid = torch.tensor([L], device="cuda")
    logits, _ = eng.logits_argmax(hn.view(1, L, -1)[:, -1])
    ltol = logit_tol(dt, dbg["prefill_logits"])
    report("prefill logits, text longer than the window", logits, dbg["prefill_logits"], ltol, 0.0)
    for i in range(n_new):                                    # teacher-forced with the oracle's tokens: every step's logits
        tok = torch.tensor([int(ref_ids[0, i])], dtype=torch.int64, device="cuda")
        posn = ts.n_valid.clone(); ts.n_valid += 1
        h = eng.text_forward(eng.embed_tokens(tok), posn, ts, mm, Lq=1)
        lg, _ = eng.logits_argmax(h)
        report(f"decode step {i} logits, window 4", lg, dbg["step_logits"][i], ltol, 0.0)


def test_batch_of_videos_one_tower_pass_and_the_batch_token_budget():
    """multimodal.py:157-180 on the HIP engine: a batch of two videos goes through SigLIP / Whisper in ONE pass (the concatenated frames /
    windows) and the token-budget rule counts the frames of the WHOLE batch — 3 + 4 frames cross the (lowered) budget that neither
    video crosses alone.  `encode_videos` against the oracle's batched evaluation (masks bit-exact), first greedy tokens of `generate`
    against the oracle's batched greedy loop, and the number of tower launches (one pass = as many as for one 7-frame video)."""
    from vidi_amd.config import tiny
    from vidi_amd.model import VidiForCausalLM
    from vidi_amd import hip
    dt = torch.bfloat16
    cfg = tiny(mm_max_tokens_base=75)
    eng, w32 = make(cfg, dt, seed=4)
    ocfg = oracle_cfg(cfg)
    model = VidiForCausalLM.__new__(VidiForCausalLM)
    model.config, model.dtype, model.device, model.engine = cfg, dt, torch.device("cuda"), eng
    from types import SimpleNamespace
    model.generation_config = SimpleNamespace(eos_token_id=cfg.eos_token_id, pad_token_id=0)
    model.model = None
    S = cfg.vis_image_size
    vids = [seeded((n, 3, S, S), 300 + n, 0.5).clamp(-1, 1).to(dt) for n in (3, 4)]
    mels = [seeded((1, cfg.aud_num_mel_bins, cfg.aud_nb_max_frames), 310 + i, 0.3).to(dt) for i in range(2)]
    sizes = [100, 83]
    fb, mb = O.encode_video_images([v.float() for v in vids], w32, ocfg)
    ab, amb = O.encode_video_audios([m.float() for m in mels], sizes, w32, ocfg)
    alone, _ = O.encode_video_images([vids[0].float()], w32, ocfg)
    assert fb.shape[1] // 4 != alone.shape[1] // 3                               # the batch is pooled differently from a video alone
    timer = hip.KernelTimer()
    hip.TIMER = timer
    try:
        fi, mi, fa, ma = model.encode_videos([v.cuda() for v in vids], [m.cuda() for m in mels], sizes)
        torch.cuda.synchronize()
    finally:
        hip.TIMER = None
    n_batch = sum(v["launches"] for v in timer.summary().values())
    timer1 = hip.KernelTimer()
    hip.TIMER = timer1
    try:
        model.encode_videos([torch.cat(vids).cuda()], [torch.cat(mels).cuda()], [183])
        torch.cuda.synchronize()
    finally:
        hip.TIMER = None
    n_one = sum(v["launches"] for v in timer1.summary().values())
    assert torch.equal(mi.cpu(), mb) and torch.equal(ma.cpu(), amb)
    report("batched encode_videos: image features", fi, fb, *tol(dt, fb.std().item(), tight=True))
    report("batched encode_videos: audio features", fa, ab, *tol(dt, ab.std().item(), tight=True))
    # one tower pass for the batch: the per-video tail (pool, projector, norms, positions) adds a few launches per video, the towers none
    assert n_batch < n_one + 40, (n_batch, n_one)
    ids = torch.tensor([[2, 21, 22, -200, 23, 24], [2, 31, -200, 32, 33, 34]])
    ref_ids, dbg = O.generate_greedy(ids, [v.float() for v in vids], [m.float() for m in mels], sizes, w32, ocfg, 4, return_debug=True)
    out = model.forward(ids, images=[v.cuda() for v in vids], audios=[m.cuda() for m in mels], audio_sizes=sizes, logits_to_keep=1)
    ref_logits = dbg["prefill_logits"]
    ltol = logit_tol(dt, ref_logits)
    report("batched forward: last-token logits of both rows", out.logits[:, -1], ref_logits, ltol, 0.0)
    got = model.generate(ids, images=[v.cuda() for v in vids], audios=[m.cuda() for m in mels], audio_sizes=sizes, max_new_tokens=4,
                         eos_token_id=999999).cpu()
    for b in range(2):
        top2 = torch.topk(ref_logits[b].float(), 2).values
        if float(top2[0] - top2[1]) > 2 * ltol:
            assert int(got[b, 0]) == int(ref_ids[b, 0])


@pytest.mark.hipgraph
def test_graph_decode_equals_eager(tiny_setup, monkeypatch):
    """The hipGraph-replayed decode (device-side cache position, vidi_attn_text_dyn) must emit exactly the
    tokens of the eager per-launch loop, for a batch of two prompts of different lengths sharing one video."""
    cfg, eng, w32, dt = tiny_setup
    from vidi_amd.model import VidiForCausalLM
    from types import SimpleNamespace
    T, C = 3, 1
    px = seeded((T, 3, cfg.vis_image_size, cfg.vis_image_size), 116, 0.5).clamp(-1, 1).to(dt)
    mel = seeded((C, cfg.aud_num_mel_bins, cfg.aud_nb_max_frames), 117, 0.3).to(dt)
    model = VidiForCausalLM.__new__(VidiForCausalLM)
    model.config, model.dtype, model.device, model.engine = cfg, dt, torch.device("cuda"), eng
    model.generation_config = SimpleNamespace(eos_token_id=-12345, pad_token_id=0)     # never stop early
    model.model = None
    ids = torch.tensor([[2, 21, 22, 23, -200, 24, 25, 26], [2, 31, -200, 32, 33, 0, 0, 0]], dtype=torch.int64)
    am = torch.tensor([[1] * 8, [1] * 5 + [0] * 3], dtype=torch.int64)
    n_new = 12
    mm = model.encode_mm_state(px[None].cuda(), mel[None].cuda(), [100])
    monkeypatch.setenv("VIDI_DECODE_GRAPH", "0")
    eager = model.generate(ids, attention_mask=am, mm_state=mm, max_new_tokens=n_new, do_sample=False).cpu()
    monkeypatch.setenv("VIDI_DECODE_GRAPH", "1")
    monkeypatch.setenv("VIDI_DECODE_GRAPH_MIN", "2")
    graph = model.generate(ids, attention_mask=am, mm_state=mm, max_new_tokens=n_new, do_sample=False).cpu()
    assert eager.shape == graph.shape == (2, n_new)
    assert torch.equal(eager, graph), f"graph decode {graph.tolist()} != eager {eager.tolist()}"


def test_batched_queries_share_one_video(tiny_setup):
    """BASELINE config 5 shape: several prompts of different lengths (right-padded) against ONE encoded video.
    Every row's next-token logits must match the same prompt run alone (padding must be invisible)."""
    cfg, eng, w32, dt = tiny_setup
    from vidi_amd.model import VidiForCausalLM
    from types import SimpleNamespace
    px = seeded((3, 3, cfg.vis_image_size, cfg.vis_image_size), 126, 0.5).clamp(-1, 1).to(dt)
    mel = seeded((1, cfg.aud_num_mel_bins, cfg.aud_nb_max_frames), 127, 0.3).to(dt)
    model = VidiForCausalLM.__new__(VidiForCausalLM)
    model.config, model.dtype, model.device, model.engine = cfg, dt, torch.device("cuda"), eng
    model.generation_config = SimpleNamespace(eos_token_id=-12345, pad_token_id=0)
    model.model = None
    mm = model.encode_mm_state(px[None].cuda(), mel[None].cuda(), [100])
    prompts = [[2, 21, 22, 23, -200, 24, 25, 26], [2, 31, -200, 32], [2, 41, 42, -200, 43, 44, 45, 46, 47, 48],
               [2, -200, 51], [2, 61, 62, 63, 64, -200, 65], [2, 71, -200, 72, 73, 74], [2, 81, 82, -200, 83], [2, 91, -200, 92, 93]]
    L = max(len(p) for p in prompts)
    ids = torch.zeros((len(prompts), L), dtype=torch.int64)
    am = torch.zeros((len(prompts), L), dtype=torch.int64)
    for i, p in enumerate(prompts):
        ids[i, : len(p)] = torch.tensor(p); am[i, : len(p)] = 1
    out = model.forward(ids, attention_mask=am, mm_state=mm)
    lb = out.logits.float().cpu()                                  # [B, L-1, V] (the <image> position is cut)
    for i, p in enumerate(prompts):
        single = model.forward(torch.tensor([p]), mm_state=mm).logits.float().cpu()[0]
        n = len(p) - 1
        atol, rtol = tol(dt, single.std().item())
        report(f"batched row {i}", lb[i, :n], single, 3 * atol, rtol)
    toks = model.generate(ids, attention_mask=am, mm_state=mm, max_new_tokens=4, do_sample=False).cpu()
    assert toks.shape == (len(prompts), 4)


def test_ragged_batch_runs_on_the_valid_positions_only(tiny_setup, monkeypatch):
    """K2 varlen (xattn.py:36-103 `_unpad_xattn_input` + flash_attn_varlen_func): a right-padded batch of 8 prompts runs every text-side
    kernel on its 50 valid positions, not on the 8 x 10 = 80 padded ones (VIDI_TEXT_VARLEN=1, the default) — same logits at the valid
    positions as the padded arm (VIDI_TEXT_VARLEN=0; both arms are held to single-prompt runs in test_batched_queries_share_one_video),
    zeros at the pad positions, the same text K/V cache rows and the same greedy tokens."""
    cfg, eng, w32, dt = tiny_setup
    from vidi_amd.model import VidiForCausalLM, strip_image_token
    from types import SimpleNamespace
    monkeypatch.setenv("VIDI_TEXT_VARLEN", "0")
    eng0, _ = make(cfg, dt)
    assert eng.text_varlen and not eng0.text_varlen
    px = seeded((3, 3, cfg.vis_image_size, cfg.vis_image_size), 126, 0.5).clamp(-1, 1).to(dt)
    mel = seeded((1, cfg.aud_num_mel_bins, cfg.aud_nb_max_frames), 127, 0.3).to(dt)
    prompts = [[2, 21, 22, 23, -200, 24, 25, 26], [2, 31, -200, 32], [2, 41, 42, -200, 43, 44, 45, 46, 47, 48, 49],
               [2, -200, 51], [2, 61, 62, 63, 64, -200, 65], [2, 71, -200, 72, 73, 74], [2, 81, 82, -200, 83], [2, 91, -200, 92, 93]]
    L = max(len(p) for p in prompts)
    ids = torch.zeros((len(prompts), L), dtype=torch.int64)
    am = torch.zeros((len(prompts), L), dtype=torch.int64)
    for i, p in enumerate(prompts):
        ids[i, : len(p)] = torch.tensor(p); am[i, : len(p)] = 1
    outs = []
    for e in (eng, eng0):
        model = VidiForCausalLM.__new__(VidiForCausalLM)
        model.config, model.dtype, model.device, model.engine = cfg, dt, torch.device("cuda"), e
        model.generation_config = SimpleNamespace(eos_token_id=-12345, pad_token_id=0)
        model.model = None
        mm = model.encode_mm_state(px[None].cuda(), mel[None].cuda(), [100])
        o = model.forward(ids, attention_mask=am, mm_state=mm)
        toks = model.generate(ids, attention_mask=am, mm_state=mm, max_new_tokens=4, do_sample=False).cpu()
        ts = o.past_key_values
        outs.append((o.logits.float().cpu(), ts.kc.float().cpu(), ts.vc.float().cpu(), toks))
    _, mask, _ = strip_image_token(ids, am)
    (la, ka, va, ta), (lb, kb, vb, tb) = outs
    assert int(mask.sum()) == sum(len(p) - 1 for p in prompts) < mask.numel()
    at, rt = tol(dt, lb[mask].std().item(), tight=True)
    report("varlen vs padded: logits at the valid positions", la[mask], lb[mask], at, rt)
    assert float(la[~mask].abs().max()) == 0.0                                   # pad positions: never computed
    km = mask[None, :, :, None].expand(ka.shape[0], -1, -1, ka.shape[-1])
    report("varlen vs padded: text K cache rows", ka[:, :, : mask.shape[1]][km], kb[:, :, : mask.shape[1]][km], *tol(dt, 1.0, tight=True))
    report("varlen vs padded: text V cache rows", va[:, :, : mask.shape[1]][km], vb[:, :, : mask.shape[1]][km], *tol(dt, 1.0, tight=True))
    # the same first greedy token wherever the padded arm's top-2 margin decides it beyond the logit bound asserted above (twice the bound:
    # either arm may move either logit by it); where it does not, each arm's token is within that distance of the other arm's best.  Prompt 4
    # in fp16 is such a row: tokens 443 and 433 tie exactly in the varlen arm and are one fp16 ulp (0.0005) apart in the padded one, against a
    # bound of 0.005 — which of the two wins there is decided by one rounding anywhere upstream.  The other 7 rows have margins of 0.05 .. 0.29.
    rows = torch.arange(len(prompts))
    last = mask.long().cumsum(1).argmax(1)                                       # each prompt's last valid position
    a_last, b_last = la[rows, last], lb[rows, last]
    top2 = b_last.topk(2, dim=1).values
    slack = 2 * (at + rt * top2[:, 0].abs())
    decided = (top2[:, 0] - top2[:, 1]) > slack
    assert int(decided.sum()) >= len(prompts) - 1, decided.tolist()
    assert torch.equal(ta[decided, 0], tb[decided, 0]), (ta.tolist(), tb.tolist())
    assert bool((b_last[rows, ta[:, 0]] >= top2[:, 0] - slack).all()) and bool((a_last[rows, tb[:, 0]] >= a_last.max(dim=1).values - slack).all()), \
        (ta.tolist(), tb.tolist())


def test_real_dims_two_layers():
    """Gemma2-9B layer dims (H=3584, 16/8 heads x 256, I=14336), 2 layers, tiny towers: mm stream + text"""
    from vidi_amd.config import tiny
    dt = torch.bfloat16
    cfg = tiny(hidden_size=3584, intermediate_size=14336, num_attention_heads=16, num_key_value_heads=8, head_dim=256,
               query_pre_attn_scalar=256.0, sliding_window=4096, num_hidden_layers=2, vocab_size=1024)
    eng, w32 = make(cfg, dt, seed=5)
    ocfg = oracle_cfg(cfg)
    H = cfg.hidden_size
    Nv, Na = 300, 40
    img = seeded((1, Nv, H), 108, cfg.mm_std).to(dt); aud = seeded((1, Na, H), 109, cfg.mm_std).to(dt)
    imask = torch.ones((1, Nv), dtype=torch.bool); amask = torch.ones((1, Na), dtype=torch.bool)
    ids = torch.tensor([[2, 31, -200, 32, 33, 34, 35, 36, 37, 38, 39]], dtype=torch.int64)
    href, caches, am = _run_oracle_prefill(w32, ocfg, ids, img.float(), imask, aud.float(), amask)
    mm = eng.mm_stream_prefill(img[0].cuda(), imask[0].to(torch.uint8).cuda(), aud[0].cuda(), amask[0].to(torch.uint8).cuda(),
                               pre_normalized=False)
    nkv, hd = cfg.num_key_value_heads, cfg.head_dim
    kref, _ = caches.image[1]
    kc = mm.kc[1].reshape(nkv, -1, hd)[:, :Nv].permute(1, 0, 2).reshape(Nv, -1)
    report("real-dims image K cache L1", kc, kref[0], 3e-2 * kref.std().item(), 3e-2)
    from vidi_amd.model import strip_image_token
    idt, mask, pos_ids = strip_image_token(ids)
    ts = eng.new_text_state(1, 16)
    hn = eng.text_forward(eng.embed_tokens(idt.cuda()), pos_ids.reshape(-1).cuda(), ts, mm, Lq=idt.shape[1], new_mask=mask.cuda())
    report("real-dims text hidden", hn, href[0], 5e-2 * href.std().item(), 4e-2)         # 39 k values behind K = 3 584 / 14 336 contractions: 0.65 used
    # one decode step on top (gemv path + cached cross attention)
    nxt = torch.tensor([41], dtype=torch.int64)
    e = torch.nn.functional.embedding(nxt[:, None], w32["model.embed_tokens.weight"])
    tm = torch.cat([am, torch.ones(1, 1, dtype=torch.bool)], dim=1)
    p = torch.tensor([[idt.shape[1]]])
    href2 = O.model_forward(e, p, tm, img.float(), imask, aud.float(), amask, w32, ocfg, caches, idt.shape[1])
    hn2 = eng.text_forward(eng.embed_tokens(nxt.cuda()), p.reshape(-1).cuda(), ts, mm, Lq=1)
    report("real-dims decode hidden", hn2, href2[0], 4e-2 * href2.std().item(), 4e-2)


def test_generate_do_sample(tiny_setup):
    """do_sample=True: top_k=1 must reproduce greedy; a seeded generator is reproducible; tokens stay in-vocabulary"""
    cfg, eng, w32, dt = tiny_setup
    from types import SimpleNamespace
    from vidi_amd.model import VidiForCausalLM
    model = VidiForCausalLM.__new__(VidiForCausalLM)
    model.config, model.dtype, model.device, model.engine = cfg, dt, torch.device("cuda"), eng
    model.generation_config = SimpleNamespace(eos_token_id=cfg.eos_token_id, pad_token_id=0)
    model.model = None
    px = seeded((3, 3, cfg.vis_image_size, cfg.vis_image_size), 206, 0.5).clamp(-1, 1).to(dt)
    mel = seeded((1, cfg.aud_num_mel_bins, cfg.aud_nb_max_frames), 207, 0.3).to(dt)
    ids = torch.tensor([[2, 21, 22, 23, -200, 24, 25, 26]], dtype=torch.int64)
    st = model.encode_mm_state(px[None].cuda(), mel[None].cuda(), [100])
    # top_k=1 keeps the maximum and everything tied with it (HF semantics; bf16 logits over a 512-token vocabulary do tie):
    # the drawn token must carry the maximal logit, and equal the greedy token when the maximum is unique
    logits = model.forward(ids, mm_state=st, logits_to_keep=1).logits[0, -1].float()
    greedy = model.generate(ids, mm_state=st, max_new_tokens=1, do_sample=False, eos_token_id=-1)
    k1 = model.generate(ids, mm_state=st, max_new_tokens=1, do_sample=True, top_k=1, eos_token_id=-1)
    assert float(logits[int(k1[0, 0])]) == float(logits.max())
    if int((logits == logits.max()).sum()) == 1:
        assert torch.equal(greedy, k1)
    g = lambda: torch.Generator(device="cuda").manual_seed(11)                      # noqa: E731
    a = model.generate(ids, mm_state=st, max_new_tokens=5, do_sample=True, temperature=1.5, top_p=0.95, generator=g(), eos_token_id=-1)
    b = model.generate(ids, mm_state=st, max_new_tokens=5, do_sample=True, temperature=1.5, top_p=0.95, generator=g(), eos_token_id=-1)
    assert torch.equal(a, b) and int(a.min()) >= 0 and int(a.max()) < cfg.vocab_size


def test_engine_switch_arms_agree(tiny_setup, monkeypatch):
    """The baseline arm of every engine switch (what tools/ab_*.py time against) computes the same function: one
    video, prefill + teacher-forced decode steps on the default engine and on one built with every switch at 0.  The two arms differ in
    summation order and in weight roundings (LayerNorm and repeat_kv folds): hidden states and stream caches within the model-level
    tolerance."""
    cfg, eng, w32, dt = tiny_setup
    names = {"ln_fold": "VIDI_LN_FOLD", "attn_rm": "VIDI_ATTN_RM", "stream_norm2": "VIDI_STREAM_NORM2", "fold_repkv": "VIDI_FOLD_REPKV",
             "decode_attn": "VIDI_DECODE_ATTN", "cross_dual": "VIDI_CROSS_DUAL", "decode_norm_gemv": "VIDI_DECODE_NORM_GEMV",
             "decode_tail": "VIDI_DECODE_TAIL", "patch_loader": "VIDI_PATCH_LOADER", "attn_prescale": "VIDI_ATTN_PRESCALE"}
    assert all(getattr(eng, n) for n in names), "the fixture engine runs the default arms"
    # third arm: everything default EXCEPT the prescaled-q attention (softmax scale folded into the q projection, running maximum rounded
    # to the model dtype): its distance to the all-off arm is reported beside the default arm's, so the share of the margin that the
    # prescale form consumes is visible in the audit (the bounds that predate it are kept for this arm)
    monkeypatch.setenv("VIDI_ATTN_PRESCALE", "0")
    eng_np, _ = make(cfg, dt)
    assert not eng_np.attn_prescale and eng_np.ln_fold
    for env in names.values():
        monkeypatch.setenv(env, "0")
    eng0, _ = make(cfg, dt)
    assert not any(getattr(eng0, n) for n in names)
    T, C = 3, 1
    px = seeded((T, 3, cfg.vis_image_size, cfg.vis_image_size), 126, 0.5).clamp(-1, 1).to(dt)
    mel = seeded((C, cfg.aud_num_mel_bins, cfg.aud_nb_max_frames), 127, 0.3).to(dt)
    ids = torch.tensor([[2, 21, 22, 23, 24, 25, 26]], dtype=torch.int64).cuda()
    forced = [31, 7, 19, 44, 5]
    runs = []
    for e in (eng, eng0, eng_np):
        fi, mi = e.encode_video_images(px.cuda())
        fa, ma = e.encode_video_audios(mel.cuda(), 100)
        mm = e.mm_stream_prefill(fi, mi, fa, ma, pre_normalized=False)
        L = ids.shape[1]
        ts = e.new_text_state(1, L + len(forced) + 2)
        hn = e.text_forward(e.embed_tokens(ids), torch.arange(L, device="cuda"), ts, mm, Lq=L)
        ts.n_valid = torch.tensor([L], device="cuda")
        hs = [hn.view(1, L, -1)[:, -1].float().cpu()]
        for t in forced:
            posn = ts.n_valid.clone(); ts.n_valid += 1
            h = e.text_forward(e.embed_tokens(torch.tensor([t], device="cuda")), posn, ts, mm, Lq=1)
            hs.append(h.float().cpu())
        runs.append((mm.kc.float().cpu(), mm.vtc.float().cpu(), torch.cat(hs)))
    a, b, c = runs
    # each arm is held to `tol` against the oracle elsewhere in this file; against each other their errors add: twice those bounds
    def tol2(x, tight):
        at, rt = tol(dt, x.std().item(), tight=tight)
        return 2 * at, 2 * rt
    # the caches sit behind the encode pipeline AND the stream layers, each held to the tight bound (3 % + 2 %) against the oracle: per arm
    # the two add in quadrature (4.2 %), across the arms they add: 8 % of the spread + 4 % relative
    kv_tol = lambda x: (8e-2 * x.std().item(), 4e-2) if dt == torch.bfloat16 else (1.6e-2 * x.std().item(), 8e-3)     # noqa: E731
    report("switch arms: stream K caches", a[0], b[0], *kv_tol(b[0]))
    report("switch arms: stream V caches", a[1], b[1], *kv_tol(b[1]))
    report("switch arms: prefill + decode hidden states", a[2], b[2], *tol2(b[2], False))
    # the arm without the prescaled-q form, at the same bounds: measured (profiles/r4_tolerance_audit.jsonl) it sits at 5.2 / 6.0 % of the
    # spread (bf16 K / V caches) against 5.7 / 6.2 % for the default arm — the prescale form accounts for ~0.3 % of the spread, the rest of
    # the distance between the arms is the LayerNorm / repeat_kv folds and the summation orders
    kv_old = kv_tol
    report("switch arms [prescale off vs all off]: stream K caches", c[0], b[0], *kv_old(b[0]))
    report("switch arms [prescale off vs all off]: stream V caches", c[1], b[1], *kv_old(b[1]))
    report("switch arms [prescale off vs all off]: prefill + decode hidden states", c[2], b[2], *tol2(b[2], False))


