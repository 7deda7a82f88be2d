"""CPU: scene statistics (diffuscene_amd/scene_stats.py, dsc_box_bounds_f32 / dsc_scene_stats_f32) -- no kernel is executed here.

* the two entry points are declared, exported and bound;
* the DEFINITION of dsc_scene_stats_f32 (include/diffuscene_hip.h), written out below in plain numpy, reproduces every result of the
  reference stored in tests/golden/scene_stats.npz (tools/make_golden_scene_stats.py): integers exactly, the float32 IoU matrices bit for
  bit.  This pins the definition without the reference;
* the ValueError cases, the tuple convention for fewer than two objects, categorical_kl, summarize, the packing of per-scene dicts and
  ShapeCodeIndex.model_ids.

How the reference forms ``avg_iou``: ``float(sum(iou_list)) / len(iou_list)`` over numpy.float32 scalars, starting from Python's int 0.
Under the numpy the reference pins (1.21) that sum is promoted to float64 at its first addition; the fixture records it that way whatever
numpy the tool runs with (tools/make_golden_scene_stats.py).  ``test_reference_avg_iou_is_a_float64_sum`` reproduces the stored values bit
for bit with a float64 running sum in the reference's order, and within 1e-12 in numpy's pairwise order."""
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = ("rand", "wave", "full", "padded", "hand", "tie", "e2e")


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "scene_stats.npz"))
    return {k: g[k] for k in g.files}


def numpy_scene_stats(bounds, scores, model_ids=None):
    """One scene, n valid rows: bounds (n, 6) float32, scores (n, K) -> dict.  The definition of dsc_scene_stats_f32 in numpy."""
    b = np.asarray(bounds, dtype=np.float32)
    n = b.shape[0]
    cls = np.asarray(scores).argmax(-1) if n else np.zeros((0,), np.int64)
    out = dict(class_counts=np.bincount(cls, minlength=np.asarray(scores).shape[-1]).astype(np.int32), num_intersecting=0, num_symmetry=0,
               iou_sum=0.0, overlap_sum=0.0, volume_sum=0.0, pair_iou=np.zeros((n, n), np.float32))
    if n == 0:
        return out
    vol = (b[:, 3] - b[:, 0]) * (b[:, 4] - b[:, 1]) * (b[:, 5] - b[:, 2])                  # float32
    lt = np.maximum(b[:, None, :3], b[None, :, :3])
    rb = np.minimum(b[:, None, 3:], b[None, :, 3:])
    wh = np.maximum(rb - lt, np.float32(0))
    overlap = wh[..., 0] * wh[..., 1] * wh[..., 2]
    union = np.maximum((vol[:, None] + vol[None, :]) - overlap, np.float32(1e-6))
    with np.errstate(all="ignore"):
        iou = overlap / union
    assert iou.dtype == np.float32
    upper = np.triu(np.ones((n, n), bool), 1)
    d = b.astype(np.float64)
    half, centre = (d[:, 3:] - d[:, :3]) / 2.0, (d[:, 3:] + d[:, :3]) / 2.0
    dh = np.abs(half[:, None] - half[None, :]).max(-1)
    dc = np.abs(centre[:, None] - centre[None, :])
    sym = (dh < 0.1) & ((dc[..., 0] < 0.1) | (dc[..., 2] < 0.1)) & (cls[:, None] == cls[None, :])
    if model_ids is not None:
        m = np.asarray(model_ids)
        sym &= m[:, None] == m[None, :]
    out.update(num_intersecting=int(((iou > 0) & upper).sum()), num_symmetry=int((sym & upper).sum()),
               iou_sum=float(iou[upper].astype(np.float64).sum()), overlap_sum=float(overlap[upper].astype(np.float64).sum()),
               volume_sum=float(vol.astype(np.float64).sum()), pair_iou=np.where(upper, iou, np.float32(0)))
    return out


def scenes(golden, group):
    """-> [(n, bounds (n, 6), scores (n, K), model_ids (n,))] of a group, padding cut off."""
    c = golden[group + ".counts"]
    return [(int(n), golden[group + ".bounds"][b, :n], golden[group + ".scores"][b, :n], golden[group + ".model_ids"][b, :n])
            for b, n in enumerate(c)]


def test_symbols_declared_exported_and_bound():
    from diffuscene_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "diffuscene_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(dsc_\w+)\s*\(", hdr, flags=re.M))
    lib = _lib.load()
    for name in ("dsc_box_bounds_f32", "dsc_scene_stats_f32"):
        assert name in declared, "%s not declared in include/diffuscene_hip.h" % name
        assert name in _lib.SIGNATURES and hasattr(lib, name), "%s not exported / bound" % name
    assert int(re.search(r"#define DSC_STATS_MAX_OBJECTS (\d+)", hdr).group(1)) == _lib.STATS_MAX_OBJECTS
    assert int(re.search(r"#define DSC_STATS_ONE_WAVE_MAX (\d+)", hdr).group(1)) == _lib.STATS_ONE_WAVE_MAX


def test_fixture_holds_the_cases_of_its_docstring(golden):
    from tools.make_golden_scene_stats import GROUPS as G
    for name, (nmax, counts) in G.items():
        assert golden[name + ".bounds"].shape == (len(counts), nmax, 6) and tuple(golden[name + ".counts"]) == counts
        assert golden[name + ".scores"].shape[2] == 23
    assert golden["hand.scores"].shape[2] == 1 and golden["tie.scores"].shape[2] == 3
    pad = golden["padded.bounds"]
    for b, n in enumerate(golden["padded.counts"]):
        assert np.isnan(pad[b, n:]).all() and np.isfinite(pad[b, :n]).all() and np.isnan(golden["padded.scores"][b, n:]).all()
    t = golden["hand.tuples"]
    assert t[0, 3] == 0 and t[1, 2] == 1 and np.isposinf(t[2, 4]) and np.isnan(t[6, 4])
    assert abs(golden["hand.iou"][3, 1, 2] - 0.125) < 1e-4                                 # identical boxes, yet not 1: the 1e-6 clamp decided
    assert (golden["hand.sym_jid"][4], golden["hand.sym_jid"][5], golden["hand.sym"][5]) == (1, 0, 1)
    assert golden["tie.sym"][0] == 1


@pytest.mark.parametrize("group", GROUPS)
def test_numpy_definition_reproduces_the_reference(golden, group):
    for b, (n, bd, sc, ids) in enumerate(scenes(golden, group)):
        ref, ref_iou = golden[group + ".tuples"][b], golden[group + ".iou"][b]
        got, got_jid = numpy_scene_stats(bd, sc), numpy_scene_stats(bd, sc, ids)
        assert ref[0] == n
        assert got["num_symmetry"] == golden[group + ".sym"][b] and got_jid["num_symmetry"] == golden[group + ".sym_jid"][b]
        if n < 2:
            assert tuple(ref) == (n, 1, 0, 0, 0)
            continue
        pairs = n * (n - 1) // 2
        assert ref[1] == pairs and got["num_intersecting"] / pairs == ref[3]
        assert got["pair_iou"].tobytes() == ref_iou[:n, :n].tobytes()                       # bit for bit
        assert not ref_iou[n:].any() and not ref_iou[:, n:].any()
        with np.errstate(all="ignore"):
            ratio = np.float64(got["overlap_sum"]) / (np.float64(got["volume_sum"]) - np.float64(got["overlap_sum"]))
        if np.isfinite(ref[4]):
            assert abs(ratio - ref[4]) <= 1e-4 * abs(ref[4])
        else:
            assert (np.isnan(ratio) and np.isnan(ref[4])) or ratio == ref[4]


@pytest.mark.parametrize("group", GROUPS)
def test_reference_avg_iou_is_a_float64_sum(golden, group):
    """See the module docstring: row-major float64 running sum of the float32 IoUs bit for bit, any other order within 1e-12 relative."""
    for b, (n, bd, sc, ids) in enumerate(scenes(golden, group)):
        if n < 2:
            continue
        ref = golden[group + ".tuples"][b]
        got = numpy_scene_stats(bd, sc)
        acc = 0.0
        for i in range(n):
            for j in range(i + 1, n):
                acc += float(got["pair_iou"][i, j])
        assert acc / ref[1] == ref[2]
        assert abs(got["iou_sum"] / ref[1] - ref[2]) <= 1e-12 * abs(ref[2])


def test_tuple_convention_and_ieee_division():
    from diffuscene_amd.scene_stats import reference_tuples
    z = np.zeros(5)
    rows = reference_tuples(np.array([0, 1, 2, 3, 2]), np.array([0, 0, 1, 3, 0]), np.array([0, 0, 1, 3, 0]), np.array([0, 0, .5, 3., 0]),
                            np.array([0, 0, 1., 3., 0.]), np.array([0, 0, 4., 3., 0.]))
    assert rows[0] == (0, 1, 0, 0, 0, 0) and rows[1] == (1, 1, 0, 0, 0, 0)
    assert rows[2] == (2, 1, 0.5, 1.0, 1.0 / 3.0, 1)
    assert rows[3][:4] == (3, 3, 1.0, 1.0) and np.isposinf(rows[3][4]) and np.isnan(rows[4][4])
    assert z.sum() == 0


@pytest.mark.parametrize("group", ("rand", "wave", "padded", "e2e", "tie"))
def test_summarize_and_categorical_kl_against_the_stored_values(golden, group):
    from diffuscene_amd import scene_stats as S
    rows = [tuple(t) + (int(s),) for t, s in zip(golden[group + ".tuples"], golden[group + ".sym_jid"])]
    got = S.summarize(rows)
    agg = golden[group + ".agg"]
    want = dict(num_scenes=len(rows), num_objects_mean=agg[0], num_objects_std=agg[1], num_pairs_mean=agg[2], box_iou_mean=agg[3],
                box_intersec_mean=agg[4], overlap_ratio_mean=agg[5], total_num_symmetries=int(agg[6]), total_num_pairs=int(agg[7]))
    assert got == want
    assert S.categorical_kl(golden["kl.p"], golden["kl.q"]) == golden["kl.value"]
    hist = np.stack([numpy_scene_stats(bd, sc)["class_counts"] for _, bd, sc, _ in scenes(golden, "rand")])
    assert np.array_equal(S.class_frequencies(hist), golden["kl.p"])
    assert S.categorical_kl(golden["kl.p"], golden["kl.p"]) == 0.0


def _dict(n, K=4, seed=0):
    g = np.random.default_rng(seed)
    return {"class_labels": g.normal(size=(1, n, K)).astype(np.float32), "translations": g.normal(size=(1, n, 3)).astype(np.float32),
            "sizes": g.uniform(0.1, 1, size=(1, n, 3)).astype(np.float32), "angles": g.uniform(-3, 3, size=(1, n, 1)).astype(np.float32)}


def test_pack_dicts_pads_into_one_buffer():
    from diffuscene_amd.scene_stats import pack_dicts
    ds = [_dict(3, seed=1), {k: torch.from_numpy(v) for k, v in _dict(0, seed=2).items()}, _dict(5, seed=3)]
    ids = [np.array([4, 4, 9]), np.zeros((0,), np.int64), torch.arange(5)]
    buf, B, nmax, K, has = pack_dicts(ds, ids)
    assert (B, nmax, K, has) == (3, 5, 4, True) and buf.dtype == np.float32 and buf.shape == (15 * 11 + 3 + 15,)
    sec = 15
    assert np.array_equal(buf[:sec * 3].reshape(3, 5, 3)[2], ds[2]["translations"][0])
    assert np.array_equal(buf[sec * 6:sec * 7].reshape(3, 5)[0, :3], ds[0]["angles"][0, :, 0]) and not buf[sec * 6:sec * 7].reshape(3, 5)[0, 3:].any()
    assert np.array_equal(buf[sec * 7:sec * 11].reshape(3, 5, 4)[0, :3], ds[0]["class_labels"][0])
    assert buf[sec * 11:sec * 11 + 3].view(np.int32).tolist() == [3, 0, 5]
    assert buf[sec * 11 + 3:].view(np.int32).reshape(3, 5)[0].tolist() == [4, 4, 9, 0, 0]
    assert pack_dicts(ds)[0].shape == (15 * 11 + 3,)


def test_value_errors_name_the_scene_before_any_launch(monkeypatch):
    from diffuscene_amd import _lib
    from diffuscene_amd import scene_stats as S
    monkeypatch.setattr(_lib, "fn", lambda name: pytest.fail("%s launched" % name))
    monkeypatch.setattr(S, "_device_of", lambda *a: torch.device("cpu"))                    # host checks only: nothing reaches a kernel
    bd, sc = torch.zeros(3, 4, 6), torch.zeros(3, 4, 5)
    with pytest.raises(ValueError, match="scene 1: count 5 outside"):
        S.scene_stats(bd, sc, counts=[0, 5, 4])
    with pytest.raises(ValueError, match="scene 2: count -1 outside"):
        S.box_bounds(torch.zeros(3, 4, 3), torch.zeros(3, 4, 3), torch.zeros(3, 4), counts=torch.tensor([0, 4, -1]))
    with pytest.raises(ValueError, match="2 counts for 3 scenes"):
        S.scene_stats(bd, sc, counts=[1, 2])
    with pytest.raises(ValueError, match="integer counts"):
        S.scene_stats(bd, sc, counts=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="class_scores: expected"):
        S.scene_stats(bd, torch.zeros(3, 5, 5))
    with pytest.raises(ValueError, match="bounds: expected"):
        S.scene_stats(torch.zeros(3, 4, 5), sc)
    with pytest.raises(ValueError, match="K = 0"):
        S.scene_stats(bd, torch.zeros(3, 4, 0))
    with pytest.raises(ValueError, match="model_ids: expected"):
        S.scene_stats(bd, sc, model_ids=torch.zeros(3, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="model_ids: integer"):
        S.scene_stats(bd, sc, model_ids=torch.zeros(3, 4))
    with pytest.raises(ValueError, match="cannot be converted"):
        S.scene_stats(torch.zeros(3, 4, 6, dtype=torch.complex64), sc)
    with pytest.raises(ValueError, match="cannot be converted"):
        S.scene_stats(np.array([["a"] * 6] * 4)[None], sc[:1])
    with pytest.raises(ValueError, match="above the limit"):
        S.scene_stats(torch.zeros(1, 161, 6), torch.zeros(1, 161, 2))
    with pytest.raises(ValueError, match="sizes: expected"):
        S.box_bounds(torch.zeros(3, 4, 3), torch.zeros(3, 5, 3), torch.zeros(3, 4))
    with pytest.raises(ValueError, match="angles: expected"):
        S.box_bounds(torch.zeros(3, 4, 3), torch.zeros(3, 4, 3), torch.zeros(3, 4, 2))
    bad = _dict(3)
    bad["sizes"] = bad["sizes"][:, :2]
    with pytest.raises(ValueError, match="scene 1: mismatched shapes"):
        S.scene_stats_from_dicts([_dict(2), bad])
    with pytest.raises(ValueError, match="scene 0: key 'angles' missing"):
        S.scene_stats_from_dicts([{k: v for k, v in _dict(2).items() if k != "angles"}])
    with pytest.raises(ValueError, match="scene 1: 5 classes"):
        S.scene_stats_from_dicts([_dict(2), _dict(2, K=5)])
    with pytest.raises(ValueError, match="scene 0: model_ids"):
        S.scene_stats_from_dicts([_dict(2)], model_ids=[np.array([1, 2, 3])])
    # a float64 / strided input HAS a float32 contiguous form: converted, not refused
    t = S._as_f32(torch.zeros(4, 6, dtype=torch.float64).t(), "x")
    assert t.dtype == torch.float32 and t.is_contiguous()


def test_shape_code_index_numbers_the_model_directories(monkeypatch):
    from diffuscene_amd import retrieval

    def obj(label, path=None):
        o = types.SimpleNamespace(label=label, size=np.ones(3), raw_model_norm_pc_lat32=lambda: np.zeros(32, np.float32))
        if path is not None:
            o.raw_model_path = path
        return o
    objs = [obj("bed", "/data/3D-FUTURE-model/aaa/raw_model.obj"), obj("bed", "/data/3D-FUTURE-model/bbb/raw_model.obj"), obj("chair"),
            obj("chair", "/elsewhere/aaa/raw_model.obj"), obj("chair")]
    idx = retrieval.ShapeCodeIndex(objs, "cpu")
    ids = idx.model_ids
    assert ids.dtype == torch.int32 and ids.shape == (5,)
    assert ids[0] == ids[3] and len({int(v) for v in ids}) == 4
