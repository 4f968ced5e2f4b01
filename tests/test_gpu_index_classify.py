"""Labelling every stored row (EmbeddingIndex.classify, classify_device, Clip.classify_index;
csrc/kernels/classify.hip) on the GPU.

Oracle: L = similarity(labels, rows as stored, "logits").T, [N][C], pinned bit-equal to the search; the labels and
logits are its k best per row by (score, lower index), bit for bit (index_cases.logits_oracle).  Softmax
probabilities and (M, S) are held to the float64 softmax of the same logits within B = bound_for(C, R) of
tests/index_probs_cases.py: the kernel feeds column c to lane c % 16 in ascending order and combines the 16 lanes
once, which is one span of the probability search and no merge, so that bound's span terms are this kernel's
and its merge terms are slack (embedding index, labelling stored rows).  At scale 100 on unit rows R is
up to 200.  Sigmoid probabilities are those of similarity(..., "sigmoid") bit for bit."""
import functools

import numpy as np
import pytest

from tests import index_cluster_cases as cluster
from tests import index_probs_cases as probs
from tests.index_cases import bits_equal_with_nans, logits_oracle, pattern, unit_rows

pytestmark = pytest.mark.gpu

N, CAP, SCALE = 200, 264, 100.0  # a partial last block of 64, slots beyond size
KS = (1, 5, 16)


@functools.lru_cache(maxsize=None)
def stored(E, dt):
    """The gallery [N][E] as an index of type dt stores it; shared, never written to."""
    g = unit_rows(np.random.default_rng(5100 + E), N, E)
    with cluster.index_of(g, dt, CAP) as ix:
        g = ix.rows()
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def label_rows(C, E):
    return unit_rows(np.random.default_rng(5200 + 7 * C + E), C, E)


def matrices(lab, g, scale=SCALE, bias=0.0):
    from open_clip_inference.engine import similarity
    return tuple(np.ascontiguousarray(similarity(np.ascontiguousarray(lab), g, scale, bias, a, 1).T)
                 for a in ("logits", "sigmoid"))


def assert_same(got, want, what=""):
    """Labels exactly, logits bit for bit (a NaN where the oracle has one)."""
    assert got[0].dtype == np.int64 and got[1].dtype == np.float32, what
    assert np.array_equal(got[0], want[0]), what
    bits_equal_with_nans(got[1], want[1])


def check(ix, lab, L, P, k, ok, scale=SCALE, bias=0.0, what=""):
    """classify against the oracle for the rows in ok; the empty entry everywhere else."""
    C = len(lab)
    got = ix.classify(lab, k, scale, bias, "softmax", allow=None, return_norm=True)
    want = logits_oracle(L, np.ones(C, bool), k)
    assert_same((got[0][ok], got[1][ok]), (want[0][ok], want[1][ok]), what)
    probs.check(tuple(a[ok] for a in got), L[ok], np.ones(C, bool), what)
    assert (got[0][~ok] == -1).all() and np.isneginf(got[1][~ok]).all() and (got[2][~ok] == 0).all(), what
    assert np.isneginf(got[3][~ok, 0]).all() and (got[3][~ok, 1] == 0).all(), what
    sg = ix.classify(lab, k, scale, bias, "sigmoid", return_norm=True)
    assert_same(sg[:2], got[:2], what + " sigmoid")
    assert np.isnan(sg[3]).all(), what  # no normaliser: the array stays as it was handed in
    sp = np.where(sg[0] >= 0, np.take_along_axis(P, np.maximum(sg[0], 0), 1), np.float32(0))
    bits_equal_with_nans(sg[2], sp)
    return got


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("C", [1, 5, 64, 65, 130])
@pytest.mark.parametrize("E", [16, 80])
def test_labels_logits_and_probabilities(E, C, dt):
    g, lab = stored(E, dt), label_rows(C, E)
    L, P = matrices(lab, g)
    with cluster.index_of(g, dt, CAP) as ix:
        for k in KS:
            got = check(ix, lab, L, P, k, np.ones(N, bool), what=f"E {E} C {C} {dt} k {k}")
            if k == 1:
                a = ix.assign(lab, SCALE, 0.0)
                assert_same((got[0][:, 0], got[1][:, 0]), a, "k = 1 is assign")


def special(name):
    """(rows, labels, bias): inputs where the order rule, not the score, decides."""
    g, lab = cluster.tie_case()  # labels 70 and 129 copy 3 and 64, across a tile seam
    lab, bias = lab.copy(), 0.0
    if name == "many equal":  # 20 copies of one row's nearest label, spread over three tiles: more than k
        lab[np.arange(2, 130, 7)[:20]] = lab[3]
    elif name == "nan":  # ten labels, fewer than k = 16: the NaN is an entry, the last before the padding
        lab = lab[60:70].copy()
        lab[6, 5] = np.nan
    elif name == "zero":  # the score of label 9 is exactly the bias
        lab[9], bias = 0, 0.5
    return g, lab, bias


@pytest.mark.parametrize("name", ["seam", "many equal", "nan", "zero"])
def test_ties_nan_and_zero_labels(name):
    g, lab, bias = special(name)
    L, P = matrices(lab, g, 1.0, bias)
    if name == "zero":
        assert (L[:, 9] == np.float32(0.5)).all()
    with cluster.index_of(g) as ix:
        for k in KS:
            got = check(ix, lab, L, P, k, np.ones(len(g), bool), 1.0, bias, f"{name} k {k}")
            if name == "many equal":
                assert (np.diff(got[0][10]) > 0).all() and got[0][10][0] == 2  # the copies, lowest index first
            if name == "nan" and k == 16:
                assert (got[0][:, 9] == 6).all() and np.isnan(got[1][:, 9]).all() and (got[0][:, 10:] == -1).all()


@pytest.mark.parametrize("dt", ["f32", "f16"])
def test_filters_liveness_and_the_device_form(dt):
    import torch
    from open_clip_inference.index import pack_allow
    E, C, k, fill = 80, 130, 5, 7.0
    g, lab = stored(E, dt), label_rows(C, E)
    L, P = matrices(lab, g)
    allow = pattern(N)
    allow[64:128] = False  # a whole block: the early-out path
    dead = np.array([0, 3, 130, N - 1])
    with cluster.index_of(g, dt, CAP) as ix:
        ix.remove(dead)
        ok = allow & ix.is_live()
        assert ok[[6, 129, 195]].all() and not ok[dead].any()
        host = ix.classify(lab, k, SCALE, 0.0, "softmax", allow=allow, return_norm=True)
        want = logits_oracle(L, np.ones(C, bool), k)
        assert_same((host[0][ok], host[1][ok]), (want[0][ok], want[1][ok]))
        assert_same((host[0][:, 0], host[1][:, 0]), ix.assign(lab, SCALE, 0.0, allow=allow), "assign under a filter")
        probs.check(tuple(a[ok] for a in host), L[ok], np.ones(C, bool))
        assert (host[0][~ok] == -1).all() and np.isneginf(host[1][~ok]).all() and (host[2][~ok] == 0).all()
        assert np.isneginf(host[3][~ok, 0]).all() and (host[3][~ok, 1] == 0).all()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            dl = torch.from_numpy(lab.copy()).cuda()
            da = torch.from_numpy(pack_allow(allow).view(np.int32)).cuda()
            di = torch.full((CAP, k), -2, dtype=torch.int32, device="cuda")
            ds, dp = (torch.full((CAP, k), fill, dtype=torch.float32, device="cuda") for _ in range(2))
            dn = torch.full((CAP, 2), fill, dtype=torch.float32, device="cuda")
            for d_norm in (dn.data_ptr(), 0):
                ix.classify_device(dl.data_ptr(), C, k, di.data_ptr(), ds.data_ptr(), dp.data_ptr(), SCALE, 0.0,
                                   "softmax", s.cuda_stream, d_allow=da.data_ptr(), d_norm=d_norm)
                s.synchronize()
                got = [t.cpu().numpy() for t in (di, ds, dp, dn)]
                assert np.array_equal(got[0][:N], host[0]) and (got[0][N:] == -2).all()
                for a, b in zip(got[1:], host[1:]):
                    assert np.array_equal(a[:N].view(np.uint32), b.view(np.uint32)) and (a[N:] == fill).all()


@pytest.mark.parametrize("C, k, act", [(5, 0, "softmax"), (5, 17, "softmax"), (0, 1, "softmax"), (65537, 1, "softmax"),
                                       (5, 1, 2), (5, 1, 9), (5, 1, "empty")])
def test_refusals_write_nothing(C, k, act):
    from open_clip_inference import EmbeddingIndex, _lib
    with EmbeddingIndex(16, 8) as ix:
        if act != "empty":
            ix.add(label_rows(5, 16))
        lab = np.zeros((max(C, 1), 16), np.float32)
        idx = np.full((8, 16), -2, np.int64)
        out = [np.full((8, 16), 7.0, np.float32) for _ in range(3)]
        rc = _lib.lib().clipgpu_index_classify(ix.handle, lab.ctypes.data, C, k, 1.0, 0.0,
                                               act if isinstance(act, int) else 0, None, idx.ctypes.data,
                                               *(o.ctypes.data for o in out))
        assert rc == 1  # CLIPGPU_ERR_INVALID
        assert (idx == -2).all() and all((o == 7.0).all() for o in out)


def test_clip_classify_index_is_classify_topk():
    """The facade on the seeded tiny model: the labels of classify_topk for the same images, the probabilities
    within this kernel's bound plus the search's own (the two sum in different orders)."""
    from open_clip_inference import Clip
    from tests.helpers import TEXTS, cfg_with_tokenizer, images, make_model_dir
    cfg, tj, mc = cfg_with_tokenizer()
    clip = Clip.from_local_dir(make_model_dir(cfg, seed=77, tokenizer_json=tj, model_config=mc)).build()
    ims, labels, k = images(), TEXTS[:4], 3
    scale, bias = clip._scale_bias()
    with clip.build_index(ims) as index, clip.build_label_index(labels) as label_index:
        L = matrices(label_index.rows(), index.rows(), float(scale), float(bias))[0]
        tol = 2 * probs.bound_for(len(labels), float(L.max() - L.min()))[0] * probs.HI
        got = clip.classify_index(index, label_index, k)
        want = clip.classify_topk(ims, label_index, k)
        masked = clip.classify_index(index, label_index, k, allow=np.arange(len(ims)) != 1)
    assert len(got) == len(ims) and masked[1] == [] and masked[0] == got[0]
    for a, b in zip(got, want):
        assert len(a) == k and [i for i, _ in a] == [i for i, _ in b]
        for (_, p), (_, p0) in zip(a, b):
            assert abs(p - p0) <= tol * max(p, p0) + probs.TINY, (p, p0, tol)
