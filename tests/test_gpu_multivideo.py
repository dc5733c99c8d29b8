"""A batch of DIFFERENT videos decoded together: the segmented cross-attention kernels (vidi_attn_cross_seg / vidi_attn_merge_seg) against
the one-video kernels (bit for bit) and the fp32 formulation, and the model-level batch path (one ragged prefill + one decode loop over
all rows) against the CPU oracle, the row-by-row arm (VIDI_MULTI_VIDEO=0) and itself."""
import pytest
import torch

import vidi_oracle as O
from test_gpu_kernels import _cross_ref, tol
from test_gpu_model import make, oracle_cfg
from util import logit_tol, pack_kv_cache, report, seeded

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
SHAPES = [(256, 8, 2, 50.0), (128, 2, 4, None)]          # (HD, nkv, G, softcap)


@pytest.fixture(scope="module")
def hip():
    from vidi_amd import hip as h
    h.load_library()
    return h


def r64(x):
    return (x + 63) // 64 * 64


def layout(videos):
    """videos: [(ntok, n_img, n_aud)] -> (CrossSegment list without masks / flags, total keys)"""
    from vidi_amd.shard import CrossSegment
    segs, tok0, key0 = [], 0, 0
    for ntok, ni, na in videos:
        a0 = key0 + r64(ni)
        segs.append(CrossSegment(tok0=tok0, ntok=ntok, img_start=key0, n_img=ni, aud_start=a0, n_aud=na))
        tok0 += ntok
        key0 = a0 + r64(na)
    return segs, key0


def run_seg(hip, q, kc, vtc, mask, segs, nkv, G, HD, softcap, edit_items=None):
    """the two segmented launches on NaN-filled workspaces and outputs -> (out_img, out_aud, plan)"""
    from vidi_amd.shard import plan_cross_segments
    plan = plan_cross_segments(segs, nkv, G, HD)
    items = [list(it) for it in plan.items]
    if edit_items is not None:
        edit_items(items)
    items_d = torch.tensor(items, dtype=torch.int32).cuda()
    segs_d = torch.tensor(plan.segs, dtype=torch.int32).cuda()
    opart = torch.full((plan.part_rows, HD), float("nan"), dtype=torch.float32, device="cuda")
    ml = torch.full((plan.part_rows, 2), float("nan"), dtype=torch.float32, device="cuda")
    outs = [torch.full_like(q, float("nan")) for _ in range(2)]
    for i0, n in plan.launches:
        hip.attn_cross_seg(q, kc, vtc, mask, opart, ml, items_d[i0:], n_items=n, G=G, nkv=nkv, HD=HD, ntile64=kc.shape[1], scale=HD ** -0.5,
                           softcap=softcap)
    hip.attn_merge_seg(opart, ml, segs_d, outs[0], outs[1], n_segs=len(segs), max_rows=plan.max_rows, n_tokens=q.shape[0], nkv=nkv, G=G, HD=HD)
    return outs[0], outs[1], plan


def run_one_by_one(hip, q, kc, vtc, mask, segs, plan, nkv, G, HD, softcap):
    """every (segment, modality) through vidi_attn_cross + vidi_attn_merge on the segment's own rows, with the plan's zsplit for the pair"""
    outs = [torch.full_like(q, float("nan")) for _ in range(2)]
    for si, s in enumerate(segs):
        rows = slice(s.tok0, s.tok0 + s.ntok)
        R = s.ntok * G
        Rpad = (R + 31) // 32 * 32
        for mod, (start, n, moff, zero) in enumerate(((s.img_start, s.n_img, s.img_mask, s.img_zero), (s.aud_start, s.n_aud, s.aud_mask, s.aud_zero))):
            if n == 0:
                outs[mod][rows] = 0
                continue
            z = plan.zsplit[si][mod]
            opart, ml = hip.attn_cross_workspace(z, nkv, Rpad, HD, "cuda")
            opart.fill_(float("nan")); ml.fill_(float("nan"))
            hip.attn_cross(q[rows], kc, vtc, None if moff < 0 else mask[moff:], opart, ml, R=R, Rpad=Rpad, G=G, nkv=nkv, HD=HD, ntile64=kc.shape[1],
                           key_start=start, n_keys=n, scale=HD ** -0.5, softcap=softcap, zsplit=z)
            hip.attn_merge(opart, ml, outs[mod][rows], W=z, nkv=nkv, R=R, Rpad=Rpad, G=G, HD=HD, zero_out=zero)
    return outs


def differs(a, b):
    """True when two outputs are not the same bits"""
    return not torch.equal(a.view(torch.int16), b.view(torch.int16))


def random_caches(nkv, ntile, HD, dt, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    kc = torch.randn((nkv, ntile, 64, HD), generator=g, device="cuda").to(dt)
    vtc = torch.randn((nkv, 2 * ntile, HD, 32), generator=g, device="cuda").to(dt)
    return kc, vtc, g


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("HD,nkv,G,softcap", SHAPES)
def test_segments_equal_one_video_launches_bit_for_bit(hip, dt, HD, nkv, G, softcap):
    """decode shape (R <= 32 rows per segment): 4 videos with ragged key counts — one with a key mask, one without audio keys, one whose
    image keys are all invalid (mask of zeros + zero_out) — NaN-filled workspaces and outputs"""
    import dataclasses
    toks = (1, 1, 3, 32 // G)
    segs, ntot = layout([(toks[0], 3000, 1100), (toks[1], 333, 0), (toks[2], 700, 450), (toks[3], 17, 200)])
    mask = torch.ones(ntot, dtype=torch.uint8, device="cuda")
    mask[segs[0].img_start + 5: segs[0].img_start + 3000: 7] = 0
    mask[segs[2].img_start: segs[2].img_start + 700] = 0
    segs[0] = dataclasses.replace(segs[0], img_mask=segs[0].img_start)
    segs[2] = dataclasses.replace(segs[2], img_mask=segs[2].img_start, img_zero=True)
    kc, vtc, g = random_caches(nkv, ntot // 64, HD, dt, 21)
    q = torch.randn((sum(toks), nkv * G * HD), generator=g, device="cuda").to(dt)
    oi, oa, plan = run_seg(hip, q, kc, vtc, mask, segs, nkv, G, HD, softcap)
    assert len(plan.launches) == 1 and len(plan.items) * nkv <= 256
    assert plan.zsplit[1][1] == 0 and min(z for zz in plan.zsplit for z in zz if z) >= 1 and max(z for zz in plan.zsplit for z in zz) > 1
    ri, ra = run_one_by_one(hip, q, kc, vtc, mask, segs, plan, nkv, G, HD, softcap)
    assert torch.isfinite(oi.float()).all() and torch.isfinite(oa.float()).all()
    assert not differs(oi, ri) and not differs(oa, ra)
    s1, s2 = segs[1], segs[2]
    assert float(oa[s1.tok0: s1.tok0 + s1.ntok].float().abs().max()) == 0.0            # no audio keys: zeros
    assert float(oi[s2.tok0: s2.tok0 + s2.ntok].float().abs().max()) == 0.0            # no valid image key: zeros (gemma.py:180-192)
    assert float(oi[: s1.tok0 + s1.ntok].float().abs().max(dim=1).values.min()) > 0.0         # the other rows hold values


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("HD,nkv,G,softcap", SHAPES)
def test_prefill_shape_against_the_fp32_formulation(hip, dt, HD, nkv, G, softcap):
    """20-52 tokens per segment (several 32-row tiles each) against `_cross_ref`, with the bound test_gpu_kernels.py uses for this kernel family"""
    import dataclasses
    videos = [(20, 1000, 300), (39, 333, 0), (52, 2000, 100)]
    segs, ntot = layout(videos)
    ntile = ntot // 64
    nq = nkv * G
    mask_cpu = torch.ones(ntot, dtype=torch.bool)
    a0 = segs[0].aud_start
    mask_cpu[a0: a0 + 300][torch.randperm(300, generator=torch.Generator().manual_seed(43))[:100]] = False
    segs[0] = dataclasses.replace(segs[0], aud_mask=a0)
    kc = torch.zeros((nkv, ntile, 64, HD), dtype=dt)
    vtc = torch.zeros((nkv, 2 * ntile, HD, 32), dtype=dt)
    kv = {}
    for si, s in enumerate(segs):
        for mod, (start, n) in enumerate(((s.img_start, s.n_img), (s.aud_start, s.n_aud))):
            if n:
                k = seeded((n, nkv, HD), 500 + 10 * si + mod, dtype=dt); v = seeded((n, nkv, HD), 600 + 10 * si + mod, dtype=dt)
                kk, vv = pack_kv_cache(k, v, ntile, start)
                kc += kk; vtc += vv                                  # regions are disjoint and the rest of each pack is zero
                kv[(si, mod)] = (k, v)
    q = seeded((sum(v[0] for v in videos), nq, HD), 40, dtype=dt)
    oi, oa, plan = run_seg(hip, q.reshape(-1, nq * HD).contiguous().cuda(), kc.cuda(), vtc.cuda(), mask_cpu.to(torch.uint8).cuda(), segs, nkv, G,
                           HD, softcap)
    assert max(it[9] for it in plan.items) >= 96                     # several row tiles
    for si, s in enumerate(segs):
        rows = slice(s.tok0, s.tok0 + s.ntok)
        for mod, (out, start, n) in enumerate(((oi, s.img_start, s.n_img), (oa, s.aud_start, s.n_aud))):
            if n == 0:
                assert float(out[rows].float().abs().max()) == 0.0
                continue
            k, v = kv[(si, mod)]
            ref = _cross_ref(q[rows], k, v, mask_cpu[start: start + n], HD ** -0.5, softcap, G)
            report(f"attn_cross_seg video {si} modality {mod}", out[rows], ref, *tol(dt, max(0.05, ref.std().item()), k=2))


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_videos_are_isolated_and_a_swapped_table_is_detected(hip, dt):
    """overwriting video 1's key regions leaves video 0's output bit-identical (and changes video 1's); control: with the image `key_start` of the
    two segments swapped in the table, the comparison against the one-video launches reports a mismatch"""
    HD, nkv, G, softcap = 256, 8, 2, 50.0
    segs, ntot = layout([(2, 1000, 300), (3, 1000, 300)])
    kc, vtc, g = random_caches(nkv, ntot // 64, HD, dt, 33)
    q = torch.randn((5, nkv * G * HD), generator=g, device="cuda").to(dt)
    oi, oa, plan = run_seg(hip, q, kc, vtc, None, segs, nkv, G, HD, softcap)
    ri, ra = run_one_by_one(hip, q, kc, vtc, None, segs, plan, nkv, G, HD, softcap)
    assert not differs(oi, ri) and not differs(oa, ra)
    kc2, vtc2 = kc.clone(), vtc.clone()
    t0 = segs[1].img_start // 64
    kc2[:, t0:] = torch.randn(kc2[:, t0:].shape, generator=g, device="cuda").to(dt)
    vtc2[:, 2 * t0:] = torch.randn(vtc2[:, 2 * t0:].shape, generator=g, device="cuda").to(dt)
    oi2, oa2, _ = run_seg(hip, q, kc2, vtc2, None, segs, nkv, G, HD, softcap)
    assert not differs(oi2[:2], oi[:2]) and not differs(oa2[:2], oa[:2])
    assert differs(oi2[2:], oi[2:]) and differs(oa2[2:], oa[2:])

    def swap(items):
        starts = (segs[0].img_start, segs[1].img_start)
        for it in items:
            if it[3] in starts:
                it[3] = starts[1 - starts.index(it[3])]
    oi3, oa3, _ = run_seg(hip, q, kc, vtc, None, segs, nkv, G, HD, softcap, edit_items=swap)
    assert differs(oi3, ri), "a table that points the videos at each other's image keys went unnoticed"
    assert differs(oi3[:2], ri[:2]) and differs(oi3[2:], ri[2:])
    assert not differs(oa3, ra)                                       # the audio regions were left alone


def test_a_record_outside_the_declared_buffers_is_skipped(hip):
    """a work item whose key region or partial region does not fit what the caller declared never touches memory: its partial keeps the fill"""
    HD, nkv, G, dt = 256, 8, 2, torch.bfloat16
    segs, ntot = layout([(1, 500, 0)])
    kc, vtc, g = random_caches(nkv, ntot // 64, HD, dt, 5)
    q = torch.randn((1, nkv * G * HD), generator=g, device="cuda").to(dt)

    def beyond(items):
        for it in items:
            it[4] = 64 * kc.shape[1] + 1            # n_keys one key past the end of the cache
    oi, _, _ = run_seg(hip, q, kc, vtc, None, segs, nkv, G, HD, 50.0, edit_items=beyond)
    torch.cuda.synchronize()
    assert float(oi.float().abs().max()) == 0.0     # no partial was written (the merge skips the NaN fill: m = -inf -> zeros)


# ---------------------------------------------------------------------------------------------------------------------------------------
# model level: one ragged prefill + one decode loop over all rows
# ---------------------------------------------------------------------------------------------------------------------------------------
FRAMES = (3, 4, 2)
SIZES = [100, 83, 61]
N_NEW = 4
W_SEED, IN_SEED = 4, 700          # weights / inputs: chosen on the CPU oracle so that most compared positions have a top-2 margin > 2 x logit_tol


def new_model(cfg, dt, seed=W_SEED):
    from types import SimpleNamespace
    from vidi_amd.model import VidiForCausalLM
    eng, w32 = make(cfg, dt, seed=seed)
    model = VidiForCausalLM.__new__(VidiForCausalLM)
    model.config, model.dtype, model.device, model.engine = cfg, dt, torch.device("cuda"), eng
    model.generation_config = SimpleNamespace(eos_token_id=cfg.eos_token_id, pad_token_id=0)
    model.model = None
    return model, w32


def batch_inputs(cfg, dt, audio=True, left=False, seed=IN_SEED):
    """three videos of 3 / 4 / 2 frames (with audio), ragged prompts of 7 / 5 / 6 positions (the <image> placeholder included) + attention mask"""
    S = cfg.vis_image_size
    vids = [seeded((n, 3, S, S), seed + n, 0.5).clamp(-1, 1).to(dt) for n in FRAMES]
    mels = [seeded((1, cfg.aud_num_mel_bins, cfg.aud_nb_max_frames), seed + 10 + i, 0.3).to(dt) for i in range(len(FRAMES))] if audio else None
    rows = [[2, 21, 22, -200, 23, 24, 25], [2, 31, -200, 32, 33], [2, 41, 42, 43, -200, 44]]
    L = max(len(r) for r in rows)
    ids = torch.zeros((len(rows), L), dtype=torch.int64)
    am = torch.zeros((len(rows), L), dtype=torch.int64)
    for i, r in enumerate(rows):
        sl = slice(L - len(r), L) if left else slice(0, len(r))
        ids[i, sl] = torch.tensor(r)
        am[i, sl] = 1
    return vids, mels, (SIZES if audio else None), ids, am


def oracle_run(cfg, w32, vids, mels, sizes, ids, am, n_new=N_NEW):
    return O.generate_greedy(ids, [v.float() for v in vids], None if mels is None else [m.float() for m in mels], sizes, w32, oracle_cfg(cfg),
                             n_new, attention_mask=am, return_debug=True)


def check_tokens(got, ref_ids, dbg, ltol, eos):
    """tokens equal wherever the oracle's top-2 margin exceeds 2 x logit_tol; a row is followed until its first low-margin step (from there on
    the two runs may see different contexts) or the oracle's EOS; at least half of the compared positions must carry such a margin"""
    compared = strong = 0
    for b in range(ref_ids.shape[0]):
        for t in range(min(got.shape[1], ref_ids.shape[1])):
            lg = dbg["prefill_logits"][b] if t == 0 else dbg["step_logits"][t - 1][b]
            top2 = torch.topk(lg.float(), 2).values
            compared += 1
            if float(top2[0] - top2[1]) <= 2 * ltol:
                break
            strong += 1
            assert int(got[b, t]) == int(ref_ids[b, t]), f"row {b} step {t}: {int(got[b, t])} != oracle {int(ref_ids[b, t])}"
            if int(ref_ids[b, t]) == eos:
                break
    print(f"margin rule: {strong} of {compared} compared positions above 2 x tol")
    assert 2 * strong >= compared, (strong, compared)
    return strong, compared


def gen_kw(vids, mels, sizes, am):
    return dict(images=[v.cuda() for v in vids], audios=None if mels is None else [m.cuda() for m in mels], audio_sizes=sizes, attention_mask=am)


def last_logits(out, am):
    """logits of every row's last attended token from the right-padded [B, L, V] frame"""
    n = am.sum(-1)
    return out.logits[torch.arange(am.shape[0]), (n - 1 - 1).to(out.logits.device)]       # (- 1 more: the <image> placeholder is not a position)


def _model_case(cfg, dt, audio, left, seed=W_SEED):
    model, w32 = new_model(cfg, dt, seed=seed)
    vids, mels, sizes, ids, am = batch_inputs(cfg, dt, audio=audio, left=left)
    ref_ids, dbg = oracle_run(cfg, w32, vids, mels, sizes, ids, am)
    ref_logits = dbg["prefill_logits"]
    ltol = logit_tol(dt, ref_logits)
    out = model.forward(ids, **gen_kw(vids, mels, sizes, am))
    from vidi_amd.engine import MMBatchState
    assert isinstance(out.past_image_key_values, MMBatchState) and out.past_image_key_values.n_videos == 3
    report("multi-video forward: last-token logits", last_logits(out, am), ref_logits, ltol, 0.0)
    got = model.generate(ids, max_new_tokens=N_NEW, eos_token_id=999999, **gen_kw(vids, mels, sizes, am)).cpu()
    assert got.shape == (3, N_NEW)
    check_tokens(got, ref_ids, dbg, ltol, cfg.eos_token_id)
    return model, w32, (vids, mels, sizes, ids, am), (ref_ids, dbg, ltol), got


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("audio", [True, False], ids=["audio", "noaudio"])
def test_three_videos_ragged_prompts_against_the_oracle(dt, audio):
    from vidi_amd.config import tiny
    _model_case(tiny(), dt, audio, left=False)


def test_vidi_7b_left_padded_batch_against_the_oracle():
    """Vidi-7B wiring: head dim 128, no softcap, a LEFT-padded batch (what mistral.py:366-373 demands for batched generation)"""
    from vidi_amd.config import tiny_7b
    _model_case(tiny_7b(), torch.bfloat16, True, left=True, seed=3)


class NamedTimer:
    """hip.KernelTimer that also keeps the entry-point names"""

    def __new__(cls):
        from vidi_amd import hip

        class _T(hip.KernelTimer):
            def __init__(self):
                super().__init__()
                self.names = []

            def run(self, name, a, fn, *stated):
                self.names.append(name)
                return super().run(name, a, fn, *stated)
        return _T()


def timed(fn):
    from vidi_amd import hip
    t = NamedTimer()
    hip.TIMER = t
    try:
        r = fn()
        torch.cuda.synchronize()
    finally:
        hip.TIMER = None
    return r, t.names


ENCODE_LAUNCHES = ("vidi_attn_self", "vidi_attn_self_rm", "vidi_patch_embed", "vidi_im2col_patch", "vidi_mel_transpose_pad", "vidi_gemm_kv_cache",
                   "vidi_pool_s2d", "vidi_add_pos")


@pytest.fixture(scope="module")
def resident():
    """one model, its oracle run and ONE resident batch state for the tests below"""
    from types import SimpleNamespace
    from vidi_amd.config import tiny
    from vidi_amd.engine import MMBatchState
    dt = torch.bfloat16
    cfg = tiny()
    model, w32, (vids, mels, sizes, ids, am), (ref_ids, dbg, ltol), got = _model_case(cfg, dt, True, left=False)
    kw = gen_kw(vids, mels, sizes, am)
    st, enc_names = timed(lambda: model.encode_mm_batch(kw["images"], kw["audios"], sizes))
    assert isinstance(st, MMBatchState) and set(enc_names) & set(ENCODE_LAUNCHES)
    run = lambda n=N_NEW, **k: model.generate(ids, attention_mask=am, mm_state=st, max_new_tokens=n, eos_token_id=999999, **k)   # noqa: E731
    return SimpleNamespace(cfg=cfg, dt=dt, model=model, ids=ids, am=am, sizes=sizes, kw=kw, st=st, run=run, got=got, ref_ids=ref_ids, dbg=dbg, ltol=ltol)


def test_resident_state_is_not_re_encoded(resident):
    """(7) two generate() calls on one resident state give the same tokens and the second runs no tower / stream launch"""
    r = resident
    st = r.st
    assert st.image_features.shape[0] == 3 and st.image_attention_mask.dtype == torch.bool and st.audio_features.shape[0] == 3
    a = r.run().cpu()
    b, names = timed(r.run)
    assert torch.equal(a, b.cpu()) and torch.equal(a, r.got)
    assert not set(names) & set(ENCODE_LAUNCHES), sorted(set(names) & set(ENCODE_LAUNCHES))
    assert names.count("vidi_attn_cross_seg") == r.cfg.num_hidden_layers * N_NEW == names.count("vidi_attn_merge_seg")
    assert len(st.plans) == 2                                            # one plan for the prefill, one for the decode loop


def test_decode_step_launches_four_videos_against_one(resident):
    """(8) a decode step for 4 videos records fewer than twice the launches of a decode step for one video (row by row: 4 x)"""
    r = resident
    model, cfg, kw = r.model, r.cfg, r.kw
    v4 = seeded((3, 3, cfg.vis_image_size, cfg.vis_image_size), 777, 0.5).clamp(-1, 1).to(r.dt)
    m4 = seeded((1, cfg.aud_num_mel_bins, cfg.aud_nb_max_frames), 778, 0.3).to(r.dt)
    st4 = model.encode_mm_batch(kw["images"] + [v4.cuda()], kw["audios"] + [m4.cuda()], r.sizes + [90])
    ids4, am4 = torch.cat([r.ids, r.ids[1:2]]), torch.cat([r.am, r.am[1:2]])
    run4 = lambda n: model.generate(ids4, attention_mask=am4, mm_state=st4, max_new_tokens=n, eos_token_id=999999)      # noqa: E731
    run4(2)
    _, n2 = timed(lambda: run4(2))
    _, n3 = timed(lambda: run4(3))
    step_batch = len(n3) - len(n2)
    one = model.encode_mm_state([kw["images"][0]], [kw["audios"][0]], [r.sizes[0]])
    ids1 = r.ids[:1, : int(r.am[0].sum())]
    run1 = lambda n: model.generate(ids1, mm_state=one, max_new_tokens=n, eos_token_id=999999)      # noqa: E731
    run1(2)
    _, m2 = timed(lambda: run1(2))
    _, m3 = timed(lambda: run1(3))
    step_one = len(m3) - len(m2)
    print(f"launches per decode step: {step_batch} for 4 videos together, {step_one} for one video")
    assert 0 < step_one and 0 < step_batch < 2 * step_one, (step_batch, step_one)


def test_per_step_scores_for_rows_that_stop_at_different_steps(resident):
    """(9) return_dict_in_generate + output_scores: HF-shaped per-step [B, V] tuples although row 0 stops first (the row-by-row path raises
    NotImplementedError there)"""
    r = resident
    model, cfg = r.model, r.cfg
    a = r.run().cpu()
    first = a[:, 0]
    assert len(set(first.tolist())) > 1, "the rows' first tokens coincide: pick other seeds"
    out = model.generate(r.ids, attention_mask=r.am, mm_state=r.st, max_new_tokens=N_NEW, eos_token_id=int(first[0]), pad_token_id=0,
                         return_dict_in_generate=True, output_scores=True, output_logits=True)
    n_done = out.sequences.shape[1]
    assert n_done > 1 and int(out.sequences[0, 0]) == int(first[0]) and bool((out.sequences[0, 1:] == 0).all())
    assert isinstance(out.scores, tuple) and len(out.scores) == n_done == len(out.logits)
    assert all(s.shape == (3, cfg.vocab_size) and s.dtype == torch.float32 for s in out.scores)
    other = [i for i in range(3) if int(first[i]) != int(first[0])]
    assert torch.equal(out.sequences[other].cpu(), a[other, :n_done])
    # the same call through images= (what a caller without a resident state writes)
    out2 = model.generate(r.ids, max_new_tokens=N_NEW, eos_token_id=int(first[0]), pad_token_id=0, return_dict_in_generate=True, output_scores=True,
                          **r.kw)
    assert torch.equal(out2.sequences, out.sequences) and len(out2.scores) == n_done


def test_two_forward_calls_are_bit_identical(resident):
    """(10)"""
    r = resident
    f1 = r.model.forward(r.ids, attention_mask=r.am, mm_state=r.st).logits
    f2 = r.model.forward(r.ids, attention_mask=r.am, mm_state=r.st).logits
    assert torch.equal(f1.view(torch.int16), f2.view(torch.int16))


def test_row_by_row_arm_gives_the_same_tokens(resident, monkeypatch):
    """(11) VIDI_MULTI_VIDEO=0 runs the row-by-row path (no segmented launch) and meets the same margin rule; a resident batch state is
    refused on that arm"""
    r = resident
    monkeypatch.setenv("VIDI_MULTI_VIDEO", "0")
    rows, names0 = timed(lambda: r.model.generate(r.ids, max_new_tokens=N_NEW, eos_token_id=999999, **r.kw))
    assert "vidi_attn_cross_seg" not in names0
    check_tokens(rows.cpu(), r.ref_ids, r.dbg, r.ltol, r.cfg.eos_token_id)
    strong = [(b, t) for b in range(3) for t in range(N_NEW)
              if float(torch.topk((r.dbg["prefill_logits"][b] if t == 0 else r.dbg["step_logits"][t - 1][b]).float(), 2).values.diff().abs()) > 2 * r.ltol]
    same_prefix = [(b, t) for b, t in strong if torch.equal(rows.cpu()[b, :t], r.got[b, :t])]
    assert same_prefix and all(int(rows[b, t]) == int(r.got[b, t]) for b, t in same_prefix)
    with pytest.raises(NotImplementedError):
        r.model.generate(r.ids, attention_mask=r.am, mm_state=r.st, max_new_tokens=2)


def test_decode_graph_switch_keeps_multi_video_generate_working(resident, monkeypatch):
    """VIDI_DECODE_GRAPH=1 (graph-replayed decode steps, a one-video mode) with a multi-video batch: the batch decodes eagerly and returns the
    tokens it returns without the switch; with VIDI_MULTI_VIDEO=0 every row keeps its own graph-captured loop"""
    r = resident
    monkeypatch.setenv("VIDI_DECODE_GRAPH", "1")
    monkeypatch.setenv("VIDI_DECODE_GRAPH_MIN", "2")
    got = r.model.generate(r.ids, max_new_tokens=N_NEW, eos_token_id=999999, **r.kw).cpu()
    assert torch.equal(got, r.got)
    assert torch.equal(r.run().cpu(), r.got)
    monkeypatch.setenv("VIDI_MULTI_VIDEO", "0")
    rows = r.model.generate(r.ids, max_new_tokens=N_NEW, eos_token_id=999999, **r.kw).cpu()
    assert rows.shape == r.got.shape
    check_tokens(rows, r.ref_ids, r.dbg, r.ltol, r.cfg.eos_token_id)


def test_what_the_batch_path_refuses(resident):
    r = resident
    with pytest.raises(RuntimeError):
        r.model.engine.make_decode_graph(r.model.engine.new_text_state(3, 16), r.st, r.got[:, 0].cuda())
    with pytest.raises(ValueError):
        r.model.generate(r.ids[:2], attention_mask=r.am[:2], mm_state=r.st, max_new_tokens=2)
    with pytest.raises(NotImplementedError):
        r.model.generate(r.ids, attention_mask=r.am, mm_state=r.st, max_new_tokens=2, num_beams=2)
