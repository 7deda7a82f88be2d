"""tests/golden/scene_stats.npz: the reference's box-level scene statistics on seeded scenes (build machine only).

Usage:  python tools/make_golden_scene_stats.py        (seconds on CPU; the file it writes is byte-identical from run to run)

Calls the REAL ``computer_intersection`` / ``computer_symmetry`` / ``axis_aligned_bbox_overlaps_3d`` of the reference's
scripts/utils.py, ``categorical_kl`` of scripts/generate_diffusion.py and ``AverageAggregator`` of scene_synthesis/stats_logger.py.
"Meshes" are duck-typed objects with ``.vertices`` (8 corners), ``.faces`` (12) and ``.bounding_box.bounds``; the bounds handed over
are the float32 bounds of the fixture widened to float64, so the reference computes on exactly the numbers dsc_scene_stats_f32 reads
(its ``astype(np.float32)`` is exact and its symmetry test sees the same doubles).  Inputs and recorded results only are stored.

Groups (``<group>.<array>`` in the file; bounds (B, Nmax, 6), scores (B, Nmax, K), model_ids (B, Nmax), counts (B,); padding rows hold
NaN / -1):
  rand     K = 23, Nmax = 21, counts (0, 1, 2, 3, 12, 21)           smallest counts and the two shipped scene sizes
  wave     K = 23, Nmax = 65, counts (63, 64, 65)                  wave boundary
  full     K = 23, Nmax = 160, counts (160,)                       largest scene the project accepts
  padded   K = 23, Nmax = 24, counts (0, 1, 5, 24, 17, 2, 24)      padding must never be read
  hand     K = 1, Nmax = 3: shared face (overlap exactly 0) | two identical boxes (IoU 1) | three identical boxes (denominator 0: inf)
           | a zero-volume box beside two identical 5 mm cubes (the 1e-6 clamp decides: IoU 0.125) | a mirror pair with equal model ids
           | the same pair with different model ids | two zero-volume boxes (0 / 0: nan)
  tie      K = 3, Nmax = 3: mirror boxes whose classes differ only through tied scores (first maximum wins)
  e2e      K = 23, Nmax = 21, counts (2, 7, 12, 21, 16): parameter-level scenes (translations, sizes, angles stored too); the bounds are
           numpy's float64 corner formula rounded to float32, and every kept scene is SEPARATED: no pair has an IoU in (0, 1e-4), a
           largest gap between the boxes within 1e-4 of 0 while the IoU is 0, or |dhalf|max, |dcx|, |dcz| within 1e-4 of 0.1 -- a
           one-ulp difference in a bound cannot flip an integer.  Scenes that violate it are redrawn.
Per group: tuples (B, 5) float64 = computer_intersection's return, sym / sym_jid (B,) = computer_symmetry without / with model_jids,
iou (B, Nmax, Nmax) float32 = strict upper triangle of the reference's IoU matrix, agg (8,) = mean objects, std, mean pairs, mean IoU,
mean intersecting share, mean overlap ratio (AverageAggregator), total symmetries (with model_jids), total pairs.
kl.p / kl.q / kl.value: class frequencies of rand and padded and the reference's categorical_kl(p, q).

The reference pins numpy 1.21.  Its ``float(sum(iou_list)) / len(iou_list)`` starts from Python's int 0 and adds numpy.float32
scalars; under numpy 1.x that first addition promotes to float64 and the sum stays there, under numpy 2 (NEP 50) it would stay a float32
running sum.  So that the recorded ``avg_iou`` does not depend on the numpy this tool happens to run with, ``sum`` in the namespace of
the reference's utils module is ``sum_numpy_1`` below, which adds in the same order with the promotion of the pinned numpy.  Nothing
else the reference does here mixes Python numbers with float32 scalars.

On the random groups ``volume_sum - overlap_sum >= 0.25 * volume_sum`` is asserted, so that cancellation cannot inflate the
difference between the reference's float32 overlap sum and a float64 one.
"""
import importlib.util
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN_FILE = os.path.join(ROOT, "tests", "golden", "scene_stats.npz")
K = 23
GROUPS = {"rand": (21, (0, 1, 2, 3, 12, 21)), "wave": (65, (63, 64, 65)), "full": (160, (160,)),
          "padded": (24, (0, 1, 5, 24, 17, 2, 24)), "e2e": (21, (2, 7, 12, 21, 16))}
SEP = 1e-4


def numpy_box_bounds(translations, sizes, angles):
    """(n, 3), (n, 3), (n,) -> (n, 6) float32: min / max over the eight corners (+-size).dot(R) + translation, R about y, in float64,
    rounded once."""
    out = np.zeros((len(angles), 6), dtype=np.float32)
    signs = np.array([[(1 if m & 1 else -1), (1 if m & 2 else -1), (1 if m & 4 else -1)] for m in range(8)], dtype=np.float64)
    for k in range(len(angles)):
        th = np.float64(angles[k])
        c, s = np.cos(th), np.sin(th)
        R = np.array([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]])
        v = (signs * np.asarray(sizes[k], dtype=np.float64)).dot(R) + np.asarray(translations[k], dtype=np.float64)
        out[k, :3], out[k, 3:] = v.min(axis=0), v.max(axis=0)
    return out


def draw_scene(rng, n, num_classes=K):
    """Seeded scene of n oriented boxes on the floor of a room that grows with n; about a third of the boxes mirror an earlier one
    (same class scores, near-equal size, mirrored in x), some of those share its model id."""
    L = max(3.0, 1.3 * np.sqrt(max(n, 1)))
    tr, sz, an = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros((n,), np.float32)
    sc, ids = np.zeros((n, num_classes), np.float32), np.zeros((n,), np.int32)
    special = np.array([0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi], dtype=np.float32)
    used = set()                                      # an original is mirrored once, a mirror never (it would land on its original)
    for k in range(n):
        j = int(rng.integers(0, max(k, 1)))
        if k > 0 and rng.random() < 0.35 and abs(tr[j, 0]) > 0.8 and j not in used:
            used.update((j, k))
            sz[k] = sz[j] + rng.normal(0, 0.02, 3).astype(np.float32)
            tr[k] = (-tr[j, 0], 0, tr[j, 2] + rng.normal(0, 0.03))
            an[k] = -an[j]
            sc[k] = sc[j]
            ids[k] = ids[j] if rng.random() < 0.5 else int(rng.integers(0, 40))
        else:
            sz[k] = (rng.uniform(0.15, 0.5), rng.uniform(0.2, 0.9), rng.uniform(0.15, 0.5))
            tr[k] = (rng.uniform(-L, L), 0, rng.uniform(-L, L))
            an[k] = special[int(rng.integers(0, 5))] if rng.random() < 0.3 else rng.uniform(-np.pi, np.pi)
            sc[k] = rng.normal(0, 1, num_classes)
            ids[k] = int(rng.integers(0, 40))
        sz[k] = np.maximum(sz[k], 0.05)
        tr[k, 1] = sz[k, 1]
    return tr, sz, an, sc, ids


def separated(bounds):
    """The separation condition of the e2e scenes (module docstring) on float32 bounds (n, 6), evaluated in float64."""
    b = bounds.astype(np.float64)
    n = len(b)
    for i in range(n):
        for j in range(i + 1, n):
            lt, rb = np.maximum(b[i, :3], b[j, :3]), np.minimum(b[i, 3:], b[j, 3:])
            d = rb - lt
            if d.min() <= 0:
                if abs(d.min()) < SEP:
                    return False
            else:
                ov = d.prod()
                if ov / max(np.prod(b[i, 3:] - b[i, :3]) + np.prod(b[j, 3:] - b[j, :3]) - ov, 1e-6) < SEP:
                    return False
            dh = np.abs((b[i, 3:] - b[i, :3]) / 2 - (b[j, 3:] - b[j, :3]) / 2).max()
            dc = np.abs((b[i, 3:] + b[i, :3]) / 2 - (b[j, 3:] + b[j, :3]) / 2)
            if min(abs(dh - 0.1), abs(dc[0] - 0.1), abs(dc[2] - 0.1)) < SEP:
                return False
    return True


def build_inputs():
    """-> {group: dict(bounds, scores, model_ids, counts[, translations, sizes, angles])}, seeded."""
    groups = {}
    for gi, (name, (nmax, counts)) in enumerate(GROUPS.items()):
        B = len(counts)
        g = dict(bounds=np.full((B, nmax, 6), np.nan, np.float32), scores=np.full((B, nmax, K), np.nan, np.float32),
                 model_ids=np.full((B, nmax), -1, np.int32), counts=np.array(counts, np.int32))
        if name == "e2e":
            g.update(translations=np.full((B, nmax, 3), np.nan, np.float32), sizes=np.full((B, nmax, 3), np.nan, np.float32),
                     angles=np.full((B, nmax), np.nan, np.float32))
        for b, n in enumerate(counts):
            for attempt in range(200):
                rng = np.random.default_rng([2024, gi, b, attempt])
                tr, sz, an, sc, ids = draw_scene(rng, n)
                bd = numpy_box_bounds(tr, sz, an)
                if name != "e2e" or separated(bd):
                    break
            else:
                raise RuntimeError("no separated scene drawn for %s[%d]" % (name, b))
            g["bounds"][b, :n], g["scores"][b, :n], g["model_ids"][b, :n] = bd, sc, ids
            if name == "e2e":
                g["translations"][b, :n], g["sizes"][b, :n], g["angles"][b, :n] = tr, sz, an
        groups[name] = g

    def box(x1, y1, z1, x2, y2, z2):
        return [x1, y1, z1, x2, y2, z2]
    unit, tiny, flat = box(0, 0, 0, 1, 1, 1), box(3, 0, 0, 3.005, 0.005, 0.005), box(0, 0, 0, 1, 1, 0)
    left, right, other = box(-2, 0, 0, -1, 1, 1), box(1, 0, 0, 2, 1, 1), box(-2, 0, 3, -1, 1, 4.5)
    hand = [([unit, box(1, 0, 0, 2, 1, 1)], [0, 0]), ([unit, unit], [0, 0]), ([unit, unit, unit], [0, 0, 0]),
            ([flat, tiny, tiny], [1, 2, 2]), ([left, right, other], [5, 5, 7]), ([left, right, other], [5, 6, 7]),
            ([flat, box(5, 0, 0, 5, 1, 1)], [0, 0])]
    g = dict(bounds=np.full((len(hand), 3, 6), np.nan, np.float32), scores=np.full((len(hand), 3, 1), np.nan, np.float32),
             model_ids=np.full((len(hand), 3), -1, np.int32), counts=np.array([len(h[0]) for h in hand], np.int32))
    for b, (boxes, ids) in enumerate(hand):
        n = len(boxes)
        g["bounds"][b, :n], g["scores"][b, :n], g["model_ids"][b, :n] = np.array(boxes, np.float32), 1.0, ids
    groups["hand"] = g
    groups["tie"] = dict(bounds=np.array([[left, right, box(1, 0, 0.05, 2, 1, 1.05)]], np.float32),
                         scores=np.array([[[0.5, 0.5, 0.1], [0.1, 0.5, 0.5], [0.5, 0.5, 0.5]]], np.float32),
                         model_ids=np.array([[3, 3, 3]], np.int32), counts=np.array([3], np.int32))
    return groups


class _Box:
    def __init__(self, bounds):
        self.bounds = bounds


class BoxMesh:
    """What computer_intersection / computer_symmetry touch of a trimesh: bounding_box.bounds, len(vertices), len(faces)."""

    def __init__(self, bounds6):
        b = np.asarray(bounds6, dtype=np.float32).astype(np.float64).reshape(2, 3)
        self.bounding_box = _Box(b)
        self.vertices = np.array([[b[(m >> 0) & 1, 0], b[(m >> 1) & 1, 1], b[(m >> 2) & 1, 2]] for m in range(8)])
        self.faces = np.zeros((12, 3), dtype=np.int64)


def sum_numpy_1(values):
    """builtins.sum with the scalar promotion of numpy 1.x (module docstring): int + float32 -> float64, float64 + anything -> float64."""
    total = 0
    for v in values:
        total = total + (np.float64(v) if isinstance(v, np.floating) else v)
    return total


def _reference():
    from oracle import ref_loader
    ref_loader.prepare_reference_script_imports()
    import generate_diffusion
    import utils
    utils.sum = sum_numpy_1
    spec = importlib.util.spec_from_file_location("dsc_ref_stats_logger", os.path.join(ref_loader.REF_ROOT, "scene_synthesis", "stats_logger.py"))
    sl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sl)
    return utils, generate_diffusion.categorical_kl, sl.AverageAggregator


def run_reference(groups):
    import torch
    utils, categorical_kl, AverageAggregator = _reference()
    out = {}
    class_counts = {}
    for name, g in groups.items():
        B, nmax = g["bounds"].shape[:2]
        tuples, sym, sym_jid = np.zeros((B, 5), np.float64), np.zeros((B,), np.int32), np.zeros((B,), np.int32)
        iou = np.zeros((B, nmax, nmax), np.float32)
        agg = [AverageAggregator() for _ in range(5)]
        n_objects, total_sym, total_pairs = [], 0, 0
        hist = np.zeros((g["scores"].shape[2],), np.int64)
        for b in range(B):
            n = int(g["counts"][b])
            meshes = [BoxMesh(g["bounds"][b, k]) for k in range(n)]
            labels, jids = g["scores"][b, :n], [int(v) for v in g["model_ids"][b, :n]]
            with np.errstate(all="ignore"):
                t = utils.computer_intersection(meshes)
            tuples[b] = t
            sym[b] = utils.computer_symmetry(meshes, labels)
            sym_jid[b] = utils.computer_symmetry(meshes, labels, jids)
            if n > 1:
                bt = torch.from_numpy(g["bounds"][b, :n][None])
                m = utils.axis_aligned_bbox_overlaps_3d(bt, bt)[0][0].numpy()
                iou[b, :n, :n] = np.triu(m, 1)
                if name in ("rand", "wave", "full", "padded", "e2e"):
                    vol = np.prod(g["bounds"][b, :n, 3:] - g["bounds"][b, :n, :3], axis=1).astype(np.float64).sum()
                    ov = t[4] * vol / (1 + t[4])
                    assert vol - ov >= 0.25 * vol, (name, b, vol, ov)
            for k in range(n):
                hist[int(labels[k].argmax(-1))] += 1
            for a, v in zip(agg, t):
                a.value = v
            n_objects.append(t[0])
            total_sym += int(sym_jid[b])
            total_pairs += t[1]
        with np.errstate(all="ignore"):
            out[name + ".agg"] = np.array([agg[0].value, np.array(n_objects).std(), agg[1].value, agg[2].value, agg[3].value, agg[4].value,
                                           total_sym, total_pairs], dtype=np.float64)
        out[name + ".tuples"], out[name + ".sym"], out[name + ".sym_jid"], out[name + ".iou"] = tuples, sym, sym_jid, iou
        class_counts[name] = hist
        for k, v in g.items():
            out[name + "." + k] = v
    p = class_counts["rand"] / class_counts["rand"].sum()
    q = class_counts["padded"] / class_counts["padded"].sum()
    out["kl.p"], out["kl.q"], out["kl.value"] = p, q, np.float64(categorical_kl(p, q))
    return out


def write_npz(path, arrays):
    """np.load-compatible, compressed, and byte-identical from run to run (fixed entry order and timestamps)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    out = run_reference(build_inputs())
    write_npz(GOLDEN_FILE, out)
    print("wrote %s (%d arrays, %d bytes)" % (GOLDEN_FILE, len(out), os.path.getsize(GOLDEN_FILE)))


if __name__ == "__main__":
    main()
