"""Scene statistics after sampling on the GPU -- the stage right behind the post-filter and retrieval.

The reference scores every generated scene from its boxes alone (scripts/generate_diffusion.py:394-429,
scripts/completion_rearrange.py:431-463): number of objects and pairs, mean pairwise axis-aligned box IoU, share of intersecting
pairs, overlap ratio and number of symmetric pairs (``computer_intersection`` / ``computer_symmetry``, scripts/utils.py:559-747), plus
the categorical KL between class frequencies (generate_diffusion.py:44).  There it is a Python double loop over the objects of one
scene on the host; here B scenes with their own object counts take two launches (dsc_box_bounds_f32, dsc_scene_stats_f32).

Boxes stand in for meshes: the bounds are those of the oriented box (translation, half extents, angle about y), which contain the bounds
of any mesh retrieved into that box."""

import numpy as np
import torch

from . import _lib, ops

_KEYS = ("class_labels", "translations", "sizes", "angles")


def _as_f32(x, name, device=None):
    """numpy / torch -> contiguous float32 torch tensor (on `device` if given); ValueError for what has no float32 form."""
    if not torch.is_tensor(x):
        a = np.asarray(x)
        if a.dtype == object or a.dtype.kind not in "fiub":
            raise ValueError("%s: dtype %s cannot be converted to float32" % (name, a.dtype))
        x = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    elif x.is_complex() or x.dtype == torch.bool:
        raise ValueError("%s: dtype %s cannot be converted to float32" % (name, x.dtype))
    if device is not None:
        x = x.to(device)
    return x.to(torch.float32).contiguous()


def _counts(counts, B, nmax, device):
    """-> (int32 device tensor (B,), host int64 array); every count is checked on the host before anything is launched."""
    if counts is None:
        host = np.full((B,), nmax, dtype=np.int64)
    else:
        host = (counts.detach().cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts))
        if host.dtype.kind not in "iu":
            raise ValueError("counts: integer counts expected, got dtype %s" % host.dtype)
        host = host.astype(np.int64).reshape(-1)
    if host.shape[0] != B:
        raise ValueError("counts: %d counts for %d scenes" % (host.shape[0], B))
    for b in range(B):
        if host[b] < 0 or host[b] > nmax:
            raise ValueError("scene %d: count %d outside [0, %d]" % (b, int(host[b]), nmax))
    if torch.is_tensor(counts) and counts.device == device and counts.dtype == torch.int32 and counts.is_contiguous():
        return counts, host
    return torch.from_numpy(host.astype(np.int32)).to(device), host


def _device_of(*xs):
    for x in xs:
        if torch.is_tensor(x) and x.is_cuda:
            return x.device
    return torch.device("cuda", torch.cuda.current_device())


def box_bounds(translations, sizes, angles, counts=None):
    """Axis-aligned bounds <x1, y1, z1, x2, y2, z2> of the oriented boxes: (B, Nmax, 3) translations, (B, Nmax, 3) half extents and
    (B, Nmax) or (B, Nmax, 1) angles in metres / radians -> (B, Nmax, 6) float32 on the device.  Rows at or beyond counts[b] are not
    read; their bounds are zero."""
    dev = _device_of(translations, sizes, angles)
    tr, sz, an = _as_f32(translations, "translations", dev), _as_f32(sizes, "sizes", dev), _as_f32(angles, "angles", dev)
    if tr.dim() != 3 or tr.shape[2] != 3:
        raise ValueError("translations: expected (B, Nmax, 3), got %s" % (tuple(tr.shape),))
    B, nmax = tr.shape[0], tr.shape[1]
    if an.dim() == 3 and an.shape[2] == 1:
        an = an.reshape(an.shape[0], an.shape[1])
    if tuple(sz.shape) != (B, nmax, 3):
        raise ValueError("sizes: expected %s, got %s" % ((B, nmax, 3), tuple(sz.shape)))
    if tuple(an.shape) != (B, nmax):
        raise ValueError("angles: expected %s or %s, got %s" % ((B, nmax), (B, nmax, 1), tuple(an.shape)))
    if B < 1 or nmax < 1:
        raise ValueError("box_bounds: empty batch %s" % ((B, nmax),))
    cnt, _ = _counts(counts, B, nmax, dev)
    out = torch.empty((B, nmax, 6), dtype=torch.float32, device=dev)
    _lib.check(_lib.fn("dsc_box_bounds_f32")(tr.data_ptr(), sz.data_ptr(), an.data_ptr(), cnt.data_ptr(), B, nmax, out.data_ptr(),
                                            ops.stream_ptr()), "dsc_box_bounds_f32")
    return out


class SceneStats:
    """Device tensors of dsc_scene_stats_f32 for B scenes: counts (B,) int32, num_intersecting / num_symmetry (B,) int32, iou_sum /
    overlap_sum / volume_sum (B,) float64, class_counts (B, K) int32, pair_iou (B, Nmax, Nmax) float32 or None."""

    def __init__(self, counts, counts_host, num_intersecting, num_symmetry, iou_sum, overlap_sum, volume_sum, class_counts, pair_iou):
        self.counts, self._counts_host = counts, counts_host
        self.num_intersecting, self.num_symmetry = num_intersecting, num_symmetry
        self.iou_sum, self.overlap_sum, self.volume_sum = iou_sum, overlap_sum, volume_sum
        self.class_counts, self.pair_iou = class_counts, pair_iou

    def __len__(self):
        return int(self._counts_host.shape[0])

    def to_reference(self):
        """Per scene ``(num_objects, num_pairs, avg_iou, avg_insec, overlap_ratio, num_symmetry)``: the tuple of the reference's
        ``computer_intersection`` and the count of its ``computer_symmetry``.  Fewer than two objects: ``(n, 1, 0, 0, 0, 0)``."""
        ints = torch.stack([self.num_intersecting, self.num_symmetry]).cpu().numpy()
        sums = torch.stack([self.iou_sum, self.overlap_sum, self.volume_sum]).cpu().numpy()
        return reference_tuples(self._counts_host, ints[0], ints[1], sums[0], sums[1], sums[2])


def reference_tuples(counts, num_intersecting, num_symmetry, iou_sum, overlap_sum, volume_sum):
    """Host arithmetic of ``SceneStats.to_reference`` on numpy vectors (IEEE division: a zero denominator gives inf or nan)."""
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for b in range(len(counts)):
            n = int(counts[b])
            if n < 2:
                out.append((n, 1, 0, 0, 0, 0))
                continue
            pairs = n * (n - 1) // 2
            ov, vol = np.float64(overlap_sum[b]), np.float64(volume_sum[b])
            out.append((n, pairs, float(iou_sum[b]) / pairs, float(num_intersecting[b]) / pairs, float(ov / (vol - ov)),
                        int(num_symmetry[b])))
    return out


def scene_stats(bounds, class_scores, counts=None, model_ids=None, return_pairs=False, block_threads=0):
    """Statistics of B scenes from their bounds (B, Nmax, 6) and class scores (B, Nmax, K) -> SceneStats.  ``model_ids`` (B, Nmax)
    int32 restricts symmetric pairs to equal retrieved models (the reference's ``model_jids``); ``return_pairs`` also returns the
    per-pair IoU matrix.  ``block_threads``: 0 = chosen by Nmax, or 64 / 256 (same bits either way)."""
    dev = _device_of(bounds, class_scores)
    bd, sc = _as_f32(bounds, "bounds", dev), _as_f32(class_scores, "class_scores", dev)
    if bd.dim() != 3 or bd.shape[2] != 6:
        raise ValueError("bounds: expected (B, Nmax, 6), got %s" % (tuple(bd.shape),))
    B, nmax = bd.shape[0], bd.shape[1]
    if sc.dim() != 3 or tuple(sc.shape[:2]) != (B, nmax):
        raise ValueError("class_scores: expected (%d, %d, K), got %s" % (B, nmax, tuple(sc.shape)))
    K = sc.shape[2]
    if K < 1:
        raise ValueError("class_scores: K = %d classes, at least 1 expected" % K)
    if B < 1 or nmax < 1:
        raise ValueError("scene_stats: empty batch %s" % ((B, nmax),))
    if nmax > _lib.STATS_MAX_OBJECTS:
        raise ValueError("scene_stats: Nmax = %d above the limit of %d objects per scene" % (nmax, _lib.STATS_MAX_OBJECTS))
    if block_threads not in (0, 64, 256):
        raise ValueError("block_threads must be 0, 64 or 256, got %r" % (block_threads,))
    mid = None
    if model_ids is not None:
        mid = model_ids if torch.is_tensor(model_ids) else torch.from_numpy(np.ascontiguousarray(np.asarray(model_ids)))
        if mid.is_floating_point() or mid.is_complex() or mid.dtype == torch.bool:
            raise ValueError("model_ids: integer ids expected, got dtype %s" % mid.dtype)
        if tuple(mid.shape) != (B, nmax):
            raise ValueError("model_ids: expected %s, got %s" % ((B, nmax), tuple(mid.shape)))
        mid = mid.to(dev, torch.int32).contiguous()
    cnt, host = _counts(counts, B, nmax, dev)
    ints = torch.empty((2, B), dtype=torch.int32, device=dev)
    sums = torch.empty((3, B), dtype=torch.float64, device=dev)
    cls = torch.empty((B, K), dtype=torch.int32, device=dev)
    pairs = torch.empty((B, nmax, nmax), dtype=torch.float32, device=dev) if return_pairs else None
    _lib.check(_lib.fn("dsc_scene_stats_f32")(
        bd.data_ptr(), sc.data_ptr(), mid.data_ptr() if mid is not None else None, cnt.data_ptr(), B, nmax, K, block_threads,
        ints[0].data_ptr(), ints[1].data_ptr(), sums[0].data_ptr(), sums[1].data_ptr(), sums[2].data_ptr(), cls.data_ptr(),
        pairs.data_ptr() if pairs is not None else None, ops.stream_ptr()), "dsc_scene_stats_f32")
    return SceneStats(cnt, host, ints[0], ints[1], sums[0], sums[1], sums[2], cls, pairs)


def pack_dicts(dicts, model_ids=None):
    """Pad the per-scene dicts (keys class_labels (1, n, K), translations (1, n, 3), sizes (1, n, 3), angles (1, n, 1) or (1, n);
    numpy or torch) into ONE host float32 buffer -> (buffer, B, Nmax, K, has_ids).  Layout: translations | sizes | angles |
    class_labels | counts | model_ids, the two integer sections stored as int32 bit patterns."""
    B = len(dicts)
    if B < 1:
        raise ValueError("scene_stats_from_dicts: no scenes")
    per = []
    for b, d in enumerate(dicts):
        row = {}
        for k in _KEYS:
            if k not in d:
                raise ValueError("scene %d: key %r missing" % (b, k))
            a = d[k].detach().cpu().numpy() if torch.is_tensor(d[k]) else np.asarray(d[k])
            if a.dtype == object or a.dtype.kind not in "fiu":
                raise ValueError("scene %d: %s has dtype %s, which cannot be converted to float32" % (b, k, a.dtype))
            if a.ndim < 2 or a.shape[0] != 1:
                raise ValueError("scene %d: %s has shape %s, leading dimension 1 expected" % (b, k, a.shape))
            row[k] = a[0].astype(np.float32)
        n = row["class_labels"].shape[0]
        row["angles"] = row["angles"].reshape(-1)
        if row["class_labels"].ndim != 2 or row["translations"].shape != (n, 3) or row["sizes"].shape != (n, 3) or row["angles"].shape != (n,):
            raise ValueError("scene %d: mismatched shapes %s" % (b, {k: row[k].shape for k in _KEYS}))
        per.append(row)
    K = per[0]["class_labels"].shape[1]
    if K < 1:
        raise ValueError("scene 0: K = 0 classes")
    for b, row in enumerate(per):
        if row["class_labels"].shape[1] != K:
            raise ValueError("scene %d: %d classes, scene 0 has %d" % (b, row["class_labels"].shape[1], K))
    counts = np.array([row["class_labels"].shape[0] for row in per], dtype=np.int32)
    nmax = max(1, int(counts.max()))
    if nmax > _lib.STATS_MAX_OBJECTS:
        raise ValueError("scene %d: %d objects, above the limit of %d" % (int(counts.argmax()), nmax, _lib.STATS_MAX_OBJECTS))
    has_ids = model_ids is not None
    if has_ids and len(model_ids) != B:
        raise ValueError("model_ids: %d lists for %d scenes" % (len(model_ids), B))
    sec = B * nmax
    buf = np.zeros((sec * (7 + K) + B + (sec if has_ids else 0),), dtype=np.float32)
    tr, sz = buf[:sec * 3].reshape(B, nmax, 3), buf[sec * 3:sec * 6].reshape(B, nmax, 3)
    an, cl = buf[sec * 6:sec * 7].reshape(B, nmax), buf[sec * 7:sec * (7 + K)].reshape(B, nmax, K)
    buf[sec * (7 + K):sec * (7 + K) + B].view(np.int32)[:] = counts
    ids = buf[sec * (7 + K) + B:].view(np.int32).reshape(B, nmax) if has_ids else None
    for b, row in enumerate(per):
        n = int(counts[b])
        tr[b, :n], sz[b, :n], an[b, :n], cl[b, :n] = row["translations"], row["sizes"], row["angles"], row["class_labels"]
        if has_ids:
            m = model_ids[b].detach().cpu().numpy() if torch.is_tensor(model_ids[b]) else np.asarray(model_ids[b])
            m = m.reshape(-1)
            if m.shape[0] != n or m.dtype.kind not in "iu":
                raise ValueError("scene %d: model_ids must be %d integers, got shape %s dtype %s" % (b, n, m.shape, m.dtype))
            ids[b, :n] = m
    return buf, B, nmax, K, has_ids


def scene_stats_from_dicts(dicts, model_ids=None, return_pairs=False, device=None):
    """Statistics of the list of per-scene dicts that ``generate_layout_batched`` / ``complete_scene_batched`` /
    ``arrange_scene_batched`` return after ``post_process``: padded and packed on the host, ONE upload, two launches.
    ``model_ids``: optional list of per-scene integer vectors (``index.model_ids[index.closest(...)]``)."""
    buf, B, nmax, K, has_ids = pack_dicts(dicts, model_ids)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    d = torch.from_numpy(buf).to(dev)
    sec = B * nmax
    tr, sz = d[:sec * 3].view(B, nmax, 3), d[sec * 3:sec * 6].view(B, nmax, 3)
    an, cl = d[sec * 6:sec * 7].view(B, nmax), d[sec * 7:sec * (7 + K)].view(B, nmax, K)
    cnt = d[sec * (7 + K):sec * (7 + K) + B].view(torch.int32)
    ids = d[sec * (7 + K) + B:].view(torch.int32).view(B, nmax) if has_ids else None
    host = buf[sec * (7 + K):sec * (7 + K) + B].view(np.int32).astype(np.int64)
    out = torch.empty((B, nmax, 6), dtype=torch.float32, device=dev)
    _lib.check(_lib.fn("dsc_box_bounds_f32")(tr.data_ptr(), sz.data_ptr(), an.data_ptr(), cnt.data_ptr(), B, nmax, out.data_ptr(),
                                            ops.stream_ptr()), "dsc_box_bounds_f32")
    st = scene_stats(out, cl, counts=host, model_ids=ids, return_pairs=return_pairs)
    return st


def out_of_room(boxes, room_mask, room_side, bounds, bbox_dim=8, class_dim=1):
    """How far the boxes of B scenes reach outside their rooms -- what ``wall_scale`` acts on, measured by the same
    launch (ops.floor_violation).  ``boxes``: (B, N, C) scenes in the network's encoding, as the loops return them; ``room_mask``: (B, 1,
    H, W) or (1, 1, H, W), inside > 0.5, rendered in the window [-room_side, room_side]^2; ``bounds``: the 12 de-normalisation bounds
    (GaussianDiffusion.box_bounds).  -> (energy (B,) f32: the summed out-of-room energy of the kept -- non-empty -- boxes, metres^2;
    share (B,) f32: the share of kept boxes with at least one of their nine footprint points outside the room, 0 for a scene that keeps
    no box)."""
    dev = _device_of(boxes, room_mask)
    x = _as_f32(boxes, "boxes", dev)
    if x.dim() != 3:
        raise ValueError("boxes: (B, N, C) scenes expected, got shape %s" % (tuple(x.shape),))
    mask = room_mask if torch.is_tensor(room_mask) else torch.from_numpy(np.ascontiguousarray(room_mask))
    energy, _, outside = ops.floor_violation(x, mask.to(dev), room_side, bounds, bbox_dim=bbox_dim, class_dim=class_dim)
    kept = (x[..., bbox_dim + class_dim - 1] < 0).sum(dim=1)
    return energy, outside.to(torch.float32) / kept.clamp(min=1).to(torch.float32)


def summarize(stats):
    """The running quantities of the reference's iou_states.txt after the last scene (its AverageAggregator means, the std of the
    object counts and the two totals).  ``stats``: a SceneStats or the list ``to_reference()`` returns."""
    rows = stats.to_reference() if isinstance(stats, SceneStats) else list(stats)
    if not rows:
        raise ValueError("summarize: no scenes")
    acc = [0, 0, 0, 0, 0]
    for r in rows:
        for k in range(5):
            acc[k] += r[k]
    m = len(rows)
    return {"num_scenes": m, "num_objects_mean": acc[0] / m, "num_objects_std": float(np.array([r[0] for r in rows]).std()),
            "num_pairs_mean": acc[1] / m, "box_iou_mean": acc[2] / m, "box_intersec_mean": acc[3] / m, "overlap_ratio_mean": acc[4] / m,
            "total_num_symmetries": int(sum(r[5] for r in rows)), "total_num_pairs": int(sum(r[1] for r in rows))}


def class_frequencies(stats):
    """Class counts summed over the scenes, normalised -> (K,) float64 numpy."""
    c = stats.class_counts if isinstance(stats, SceneStats) else stats
    c = (c.sum(dim=0).cpu().numpy() if torch.is_tensor(c) else np.asarray(c).sum(axis=0)).astype(np.float64)
    return c / c.sum()


def categorical_kl(p, q):
    """KL(p || q) between two class-frequency vectors as scripts/generate_diffusion.py:44-45 writes it (1e-6 inside both logs)."""
    p, q = np.asarray(p), np.asarray(q)
    return (p * (np.log(p + 1e-6) - np.log(q + 1e-6))).sum()
