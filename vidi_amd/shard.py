"""Frame/time-axis sharding of one video over the ranks of a node.

The reference shards its sequence-parallel *training* path the same way (`vidi/model/lmm/dattn/sequence_parallel/split.py:73-93`
cuts the token axis into contiguous per-rank ranges); inference there is single-GPU.  Here every rank takes a contiguous range of
frames and of 30-s audio windows, encodes them with the GLOBAL positions (`frame_offset`/`total_frames`, `chunk_offset`/
`audio_size`), runs the diagonal multimodal stream on its own tokens and keeps its cross-attention K/V shard resident.

Pure host integer logic: importable without a GPU (tests/test_shard.py drives it under gloo)."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Tuple


def token_budget_hw(T: int, side: int, pool: int, base: int) -> Tuple[int, int]:
    """Token-budget rule (multimodal.py:175-180 + vidi/utils.py:152-171), integer/float host math.
    Returns the `hw` the reference hands to Conv2DPool; (28,28) is its "no resize" sentinel."""
    n_tokens = T * (side + 1) * (side + 1)
    max_tokens = base * pool * pool
    if n_tokens > max_tokens:
        H = W = side + 1
        ratio = math.sqrt(max_tokens / (T * H * W))
        th, tw = int(H * ratio), int(W * ratio)
        return max(10, th - th % 2), max(10, tw - tw % 2)
    return 28, 28


def audio_token_counts(audio_size: int, cfg) -> Tuple[int, int]:
    """floor(size*1500/3000), then floor(/pool) — multimodal.py:226-227, 234-235 (same numpy float64 ops)."""
    import numpy as np
    pool_ratio = cfg.aud_max_source_positions / cfg.aud_nb_max_frames
    s1 = int(np.floor(np.array([audio_size]) * pool_ratio).astype(int)[0])
    s2 = int(np.floor(np.array([s1]) / cfg.mm_audio_pool_size).astype(int)[0])
    return s1, s2


def shard(n: int, world: int, rank: int) -> Tuple[int, int]:
    """Contiguous [start, end) of rank's share of n units; sizes differ by at most one, earlier ranks take the extra."""
    if world <= 0 or not (0 <= rank < world):
        raise ValueError(f"bad rank/world {rank}/{world}")
    base, extra = divmod(max(0, n), world)
    s = rank * base + min(rank, extra)
    return s, s + base + (1 if rank < extra else 0)


@dataclass(frozen=True)
class VideoShard:
    """What one rank encodes of a T-frame video with C audio windows."""
    f0: int
    f1: int
    c0: int
    c1: int
    total_frames: int
    total_windows: int

    @property
    def frames(self) -> int:
        return self.f1 - self.f0

    @property
    def windows(self) -> int:
        return self.c1 - self.c0


def video_shard(total_frames: int, total_windows: int, world: int, rank: int) -> VideoShard:
    f0, f1 = shard(total_frames, world, rank)
    c0, c1 = shard(total_windows, world, rank)
    return VideoShard(f0, f1, c0, c1, total_frames, total_windows)


def audio_shard_tokens(chunk_offset: int, windows_local: int, rows_per_window: int, pool: int, tokens_total: int) -> Tuple[int, int]:
    """(first global audio token, token count) of a rank that holds `windows_local` 30-s windows starting at window `chunk_offset`.
    A window gives rows_per_window encoder rows = rows_per_window // pool pooled tokens (the Conv1d has kernel == stride == pool,
    multimodal.py:231-233, so pooling never straddles a window when pool divides rows_per_window); `tokens_total` is the GLOBAL
    count floor(floor(audio_size * 1500 / 3000) / pool) (multimodal.py:226-235) and clips the last windows."""
    if rows_per_window % pool:
        raise ValueError("encoder rows per window must be a multiple of the audio pool size to shard by window")
    per = rows_per_window // pool
    tok0 = chunk_offset * per
    return tok0, max(0, min(tokens_total - tok0, windows_local * per))


def image_tokens_per_frame(cfg, budget_frames: int) -> int:
    """video tokens one frame contributes: (h / pool) * (w / pool) under the token-budget rule (Vidi1.5, `budget_frames` = the frames the
    rule counts: the whole batch's, multimodal.py:157-158, 175-180), pool * pool for Vidi-7B's learned Conv2DPool."""
    pool = cfg.mm_image_pool_size
    if cfg.arch == "mistral":
        return pool * pool
    hw = token_budget_hw(budget_frames, cfg.vis_side, pool, cfg.mm_max_tokens_base)
    h, w = hw if hw[0] != 28 else (cfg.vis_side + 1, cfg.vis_side + 1)
    return (h // pool) * (w // pool)


def gather_counts(cfg, total_frames: int, total_windows: int, audio_size: Optional[int], world: int,
                  budget_frames: Optional[int] = None) -> Tuple[List[int], List[int]]:
    """Rows every rank contributes to the all-gather of visual / audio tokens (`dist_mode = "gather_tokens"`), from host integers alone —
    no rank has to ask another how much it encoded: -> (video tokens per rank, audio tokens per rank), both in rank (= reference) order."""
    per = image_tokens_per_frame(cfg, total_frames if budget_frames is None else budget_frames) if total_frames else 0
    img = [(shard(total_frames, world, r)[1] - shard(total_frames, world, r)[0]) * per for r in range(world)]
    aud = [0] * world
    if total_windows and audio_size is not None:
        s2_total = audio_token_counts(int(audio_size), cfg)[1]
        rows = cfg.aud_max_source_positions                     # encoder rows per 30-s window
        for r in range(world):
            c0, c1 = shard(total_windows, world, r)
            aud[r] = audio_shard_tokens(c0, c1 - c0, rows, cfg.mm_audio_pool_size, s2_total)[1]
    return img, aud


def packed_partial_floats(n_modalities: int, nkv: int, rows: int, hd: int) -> int:
    """fp32 words one rank contributes to the per-layer all-gather: per modality a numerator [nkv, rows, hd] and (m, l) [nkv, rows, 2]."""
    return n_modalities * nkv * rows * (hd + 2)


def packed_offsets(slot: int, nkv: int, rows: int, hd: int) -> Tuple[int, int]:
    """(numerator offset, (m, l) offset) in fp32 words of modality slot `slot` inside one rank's packed partial."""
    base = slot * nkv * rows * (hd + 2)
    return base, base + nkv * rows * hd


def single_key_slices(slices: int, subtiles: int, min_subtiles: int = 8) -> int:
    """Split-KV key slices of a launch over ONE key region of `subtiles` 32-key sub-tiles when `slices` fit the block budget: at most
    ceil(subtiles / min_subtiles) — a region is never cut into more slices than it has runs of `min_subtiles` sub-tiles (a slice costs a
    partial and a merge step whatever its length; with the remainder spread evenly a slice may hold a few sub-tiles less) — and >= 1."""
    return max(1, min(slices, (subtiles + min_subtiles - 1) // min_subtiles))


def split_key_slices(slices: int, subtiles_a: int, subtiles_b: int, min_subtiles: int = 8):
    """Share `slices` split-KV key slices of ONE cross-attention launch between two modalities in proportion to their 32-key sub-tiles
    (the launch is as long as its slowest slice): -> (za, zb), each >= 1, za + zb <= slices, and no slice shorter than `min_subtiles`
    sub-tiles unless the modality itself is shorter (a slice costs a partial and a merge step whatever its length)."""
    if slices < 2 or subtiles_a <= 0 or subtiles_b <= 0:
        raise ValueError("two non-empty modalities and at least two slices")
    za = min(max(1, round(slices * subtiles_a / (subtiles_a + subtiles_b))), slices - 1)
    zb = slices - za
    return single_key_slices(za, subtiles_a, min_subtiles), single_key_slices(zb, subtiles_b, min_subtiles)



# ---------------------------------------------------------------------------------------------------------------------------------------
# a batch of DIFFERENT videos decoded together: the work-item plan of the segmented cross-attention (csrc/attn_cross_seg.hip)
# ---------------------------------------------------------------------------------------------------------------------------------------
XSEG_REC = 16                   # int32 words of one record of either table (include/vidi_hip.h: vidi_attn_cross_seg)


@dataclass(frozen=True)
class CrossSegment:
    """One video of the batch as the cross-attention sees it: query tokens [tok0, tok0 + ntok) of the packed text rows and, per modality, the
    key region [start, start + n) of the shared caches (start a multiple of 64), the byte offset of the region's key mask in the batch's
    mask buffer (-1: every key valid) and the `zero_out` flag (gemma.py:180-192: the sample has no valid key of the modality)."""
    tok0: int
    ntok: int
    img_start: int = 0
    n_img: int = 0
    img_mask: int = -1
    img_zero: bool = False
    aud_start: int = 0
    n_aud: int = 0
    aud_mask: int = -1
    aud_zero: bool = False


@dataclass
class CrossSegPlan:
    items: List[List[int]]              # work items, XSEG_REC ints each, in launch order (longest key slice first)
    segs: List[List[int]]               # one record per segment
    launches: List[Tuple[int, int]]     # (first item, item count) per launch: one launch unless a single slice per pair already exceeds the budget
    zsplit: List[Tuple[int, int]]       # per segment (image slices, audio slices); 0 = the segment has no key of the modality
    part_rows: int                      # rows of the partial workspaces: Opart [part_rows, HD] fp32, ML [part_rows, 2] fp32
    max_rows: int                       # largest R = ntok * G of a segment (the merge launch's row extent)
    launch_keys: List[int]              # keys each launch sweeps (a pair's keys count once, shared out over its items): the byte model's figure

    def workspace_floats(self, HD: int) -> Tuple[int, int]:
        return self.part_rows * HD, self.part_rows * 2


def share_key_slices(slices: int, subtiles: List[int], min_subtiles: int = 8) -> List[int]:
    """`split_key_slices` for n key regions: `slices` split-KV slices shared out in proportion to the regions' 32-key sub-tiles, each >= 1,
    none shorter than `min_subtiles` sub-tiles unless the region itself is.  Region by region, each takes round(what is left x its share of
    the sub-tiles that are left) and leaves one slice for every region after it — for two regions that IS split_key_slices, for one region
    min(slices, ceil(sub-tiles / min_subtiles)), the single-modality rule of the engine."""
    n = len(subtiles)
    if n == 0:
        return []
    if slices < n or any(s <= 0 for s in subtiles):
        raise ValueError("one slice per non-empty region at least")
    out, rem_z, rem_n = [], slices, sum(subtiles)
    for i, s in enumerate(subtiles):
        z = min(max(1, round(rem_z * s / rem_n)), rem_z - (n - 1 - i))
        out.append(single_key_slices(z, s, min_subtiles))
        rem_z -= z
        rem_n -= s
    return out


def plan_cross_segments(segs: List[CrossSegment], nkv: int, G: int, HD: int, budget: int = 256) -> CrossSegPlan:
    """Work-item table, segment table and workspace sizes of one segmented cross-attention launch (host integers only).

    A (segment, modality) PAIR with keys costs `row tiles x slices` blocks per kv head.  The launch gets the budget the one-video launches
    use — `budget` blocks / nkv — counted in slices of the segment with the most row tiles, and the slices are shared out over all pairs
    by `share_key_slices`; one segment therefore gets exactly the zsplit of the one-video path at the same row-tile count.  When even one
    slice per pair does not fit (many videos x long prompts), every pair gets one slice and the items are cut into several launches of
    at most `budget` blocks each.  Items are ordered longest slice first (the long videos' slices start first); the partial regions of
    the pairs are laid out back to back, [zsplit][nkv][Rpad] rows each."""
    if not segs or nkv <= 0 or G <= 0 or HD not in (128, 256):
        raise ValueError("plan_cross_segments: segments, nkv, G > 0 and HD in (128, 256)")
    per_launch = max(1, budget // nkv)                      # items (blocks per kv head) of one launch
    pairs = []                                              # (segment index, modality, sub-tiles, row tiles)
    for si, s in enumerate(segs):
        if s.ntok <= 0 or s.tok0 < 0 or s.n_img < 0 or s.n_aud < 0 or (s.img_start | s.aud_start) % 64:
            raise ValueError(f"segment {si}: tokens > 0, key counts >= 0, 64-aligned key starts")
        rt = (s.ntok * G + 31) // 32
        for mod, n in ((0, s.n_img), (1, s.n_aud)):
            if n > 0:
                pairs.append((si, mod, (n + 31) // 32, rt))
    rt_max = max((p[3] for p in pairs), default=1)
    slices = per_launch // rt_max
    if pairs and slices >= len(pairs):
        zs = share_key_slices(slices, [p[2] for p in pairs])
    else:
        zs = [1] * len(pairs)
    zsplit = [[0, 0] for _ in segs]
    base_of = [[0, 0] for _ in segs]
    items, base = [], 0
    for (si, mod, nsub, rt), z in zip(pairs, zs):
        s = segs[si]
        R = s.ntok * G
        Rpad = rt * 32
        zsplit[si][mod] = z
        base_of[si][mod] = base
        start, n, moff = (s.img_start, s.n_img, s.img_mask) if mod == 0 else (s.aud_start, s.n_aud, s.aud_mask)
        for zi in range(z):
            for t in range(rt):
                # sub-tiles of the slice's longest wave under the interleave rule (wave z * 4 + w sweeps sub-tiles wg, wg + 4 z, ...)
                items.append((-((nsub - zi * 4 + 4 * z - 1) // (4 * z)),
                              [s.tok0, R, t, start, n, moff, zi, z, base, Rpad, 1 if rt == 1 else 0] + [0] * (XSEG_REC - 11)))
        base += z * nkv * Rpad
    items.sort(key=lambda it: it[0])                        # stable: equal lengths keep (segment, modality, slice, tile) order
    items = [it[1] for it in items]
    seg_tab = []
    for si, s in enumerate(segs):
        R = s.ntok * G
        seg_tab.append([s.tok0, R, (R + 31) // 32 * 32,
                        base_of[si][0], zsplit[si][0], 1 if s.img_zero else 0,
                        base_of[si][1], zsplit[si][1], 1 if s.aud_zero else 0] + [0] * (XSEG_REC - 9))
    launches = [(i, min(per_launch, len(items) - i)) for i in range(0, len(items), per_launch)]
    launch_keys = [round(sum(it[4] / (it[7] * (it[9] // 32)) for it in items[i: i + c])) for i, c in launches]
    return CrossSegPlan(items=items, segs=seg_tab, launches=launches, zsplit=[tuple(z) for z in zsplit], part_rows=max(base, 1),
                        max_rows=max(s.ntok for s in segs) * G, launch_keys=launch_keys)
