"""One EmbeddingIndex handle through every operation (tests/index_state_cases.py has the model and the scripts).

The per-feature suites pin each operation on a fresh handle that makes one or two calls.  Here one handle lives
through a whole script, and at every check it is compared three ways:
  1. with the numpy model, which knows nothing of the library's searches: len, live, is_live, the rows as bits,
     has_codes, n_lists, and the codes against codes_oracle of the model's rows;
  2. with an anchor: the plain search against logits_oracle(similarity(queries, the model's rows));
  3. with a fresh handle of the same E, capacity and dtype built from the model (add, remove, enable_codes,
     partition): every read form must return the same bits on both.  test_two_fresh_handles_agree shows first
     that two fresh handles of equal state do agree bit for bit, probabilities included, so no tolerance is needed.
A refusal is compared too: the error is raised with the message the model predicts, and the next check shows that
nothing changed."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests import index_state_cases as cases
from tests.index_cases import assert_same, bits_equal_with_nans, logits_oracle, pattern, unit_rows
from tests.index_codes_cases import codes_oracle
from tests.index_range_cases import assert_range, range_oracle
from tests.index_state_cases import Model, Refused, centroids_for

pytestmark = pytest.mark.gpu

SCALE = 100.0
JOIN_COSINE = 0.3  # 2.7 sigma of a cosine of 80-d unit rows: a few hundred pairs of 600 rows
READS = SimpleNamespace(nq=17, k=128, pq=5, pk=10, nprobe=2, cq=5, ck=10, refine=32)
SMALL = cases.SMALL_READS
SMALL_READS = SimpleNamespace(nq=SMALL["nq"], k=SMALL["k"], pq=SMALL["nq"], pk=SMALL["k"], nprobe=SMALL["nprobe"],
                              cq=SMALL["nq"], ck=SMALL["k"], refine=SMALL["refine"])


@functools.lru_cache(maxsize=None)
def queries():
    q = unit_rows(np.random.default_rng(4242), 260, cases.E)
    q.setflags(write=False)
    return q


def logits(q, rows):
    from open_clip_inference.engine import similarity
    return similarity(np.ascontiguousarray(q), np.ascontiguousarray(rows), SCALE, 0.0, "logits", 1)


# ---- a handle built from the model, and the two ways a mutation reaches a handle --------------------------
def fresh(m):
    from open_clip_inference import EmbeddingIndex
    ix = EmbeddingIndex(m.E, m.capacity, dtype=m.dt)
    if m.size:
        ix.add(m.rows())  # the stored rows: rounding them again changes nothing
    dead = ~m.is_live()
    if m.part == "current":  # the lists hold the rows that were live when the partition was made
        early = dead & ~m.part_alive[:m.size]
        if early.any():
            ix.remove(np.flatnonzero(early))
        if m.codes:
            ix.enable_codes()
        ix.partition(m.cen)
        if (dead & ~early).any():
            ix.remove(np.flatnonzero(dead & ~early))
        return ix
    if dead.any():
        ix.remove(np.flatnonzero(dead))
    if m.codes:
        ix.enable_codes()
    return ix


def mutate(ix, step):
    import torch
    op, a = step[0], step[1:]
    if op == "add":
        ix.add(cases.rows_for(a[1], a[0], ix.E, nan=len(a) > 2))
    elif op == "add_device":
        d = torch.from_numpy(cases.rows_for(a[1], a[0], ix.E, nan=len(a) > 2)).cuda()
        try:
            ix.add_device(d.data_ptr(), a[0], torch.cuda.current_stream().cuda_stream)
        finally:
            torch.cuda.synchronize()  # d is read on the stream
    elif op == "set_rows":
        ix.set_rows(np.asarray(a[0], np.int64), cases.rows_for(a[1], len(a[0]), ix.E, nan=len(a) > 2))
    elif op == "remove":
        ix.remove(np.asarray(a[0], np.int64))
    elif op == "partition":
        ix.partition(centroids_for(a[1], a[0], ix.E))
    else:
        getattr(ix, op)()


# ---- the read forms ----------------------------------------------------------------------------------------
def attempt(fn):
    from open_clip_inference.error import ClipError
    try:
        return fn()
    except ClipError as e:
        return ("refused", str(e))


def exact(fn):
    """A range form through the smallest buffer that holds its result: refused with the total, then retried."""
    from open_clip_inference.error import ResultOverflow
    try:
        return fn(1)
    except ResultOverflow as e:
        return fn(e.needed)


def kmeans(ix, C, seed, max_iter=3):
    km = ix.kmeans(init=centroids_for(seed, C, ix.E), max_iter=max_iter)
    return km.centroids, km.labels, km.scores, km.counts, km.moved, np.int64(km.iters)


def read(ix, step, thr=None):
    """One read step of a script (or of a check) on `ix`: a tuple of arrays, or ("refused", message)."""
    q, N, op, a = queries(), len(ix), step[0], step[1:]
    allow = pattern(N) if (len(a) and a[-1] == "allow") else None
    forms = {
        "search": lambda: ix.search(q[:a[0]], a[1], SCALE, allow=allow),
        "search_probs": lambda: ix.search_probs(q[:a[0]], a[1], SCALE, 0.0, "softmax", allow=allow, return_norm=True),
        "search_probed": lambda: ix.search_probed(q[:a[0]], a[1], a[2], SCALE, return_probes=True),
        "search_coded": lambda: ix.search_coded(q[:a[0]], a[1], a[2], SCALE, return_candidates=True),
        "range_search": lambda: exact(lambda cap: ix.range_search(q[:a[0]], thr, SCALE, max_results=cap)),
        "duplicates": lambda: exact(lambda cap: ix.duplicates(JOIN_COSINE, max_pairs=cap)),
        "assign": lambda: ix.assign(centroids_for(a[1], a[0], ix.E)),
        "kmeans": lambda: kmeans(ix, a[0], a[1]),
        "rows": lambda: (ix.rows(),) if N else (),
        "rows_at": lambda: (ix.rows_at(np.arange(a[0]) * 7919 % N),) if N else (),
        "lists": lambda: ix.lists(),
    }
    return attempt(forms[op])


def check_reads(rd):
    """The read forms of one check: name -> step."""
    return {
        "search 5x10": ("search", 5, 10), "search many": ("search", rd.nq, rd.k),
        "search 5x10 allow": ("search", 5, 10, "allow"), "search many allow": ("search", rd.nq, rd.k, "allow"),
        "search_probs": ("search_probs", 5, 10), "range_search": ("range_search", 5), "duplicates": ("duplicates",),
        "assign": ("assign", 3, 1), "kmeans": ("kmeans", 4, 2), "rows_at": ("rows_at", 9), "lists": ("lists",),
        "search_probed": ("search_probed", rd.pq, rd.pk, rd.nprobe),
        "search_coded": ("search_coded", rd.cq, rd.ck, rd.refine),
    }


def bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, what):
    assert isinstance(got, tuple) and isinstance(want, tuple) and len(got) == len(want), (what, got[:2], want[:2])
    if (got and isinstance(got[0], str)) or (want and isinstance(want[0], str)):
        assert got == want, (what, got[:2], want[:2])
        return
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, i, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(bits(g), bits(w)), (what, i)


def threshold_between(L, ok, rank):
    """A threshold between two distinct logits of the live rows: below the `rank`-th largest of them."""
    v = np.unique(L[:, ok][np.isfinite(L[:, ok])])[::-1]
    if len(v) < 2:
        return 0.0
    r = min(rank, len(v) - 1)
    return float((np.float64(v[r - 1]) + np.float64(v[r])) / 2)


def device_forms(ix, m, rd, host):
    """The plain, probed and coded search through their device forms, on the current stream: what the host forms
    returned."""
    import torch
    s = torch.cuda.current_stream().cuda_stream
    dq = torch.from_numpy(queries().copy()).cuda()

    def outs(nq, *shapes):
        return [torch.full((nq, n), -7, dtype=t, device="cuda") for n, t in shapes]
    i64, f32 = torch.int64, torch.float32
    di, ds = outs(5, (10, i64), (10, f32))
    ix.search_device(dq.data_ptr(), 5, 10, di.data_ptr(), ds.data_ptr(), SCALE, 0.0, s)
    torch.cuda.synchronize()
    same((di.cpu().numpy(), ds.cpu().numpy()), host["search 5x10"], "search_device")
    if m.part == "current":
        di, ds, dp = outs(rd.pq, (rd.pk, i64), (rd.pk, f32), (rd.nprobe, i64))
        ix.search_probed_device(dq.data_ptr(), rd.pq, rd.pk, rd.nprobe, di.data_ptr(), ds.data_ptr(), SCALE, 0.0, s,
                                d_probes=dp.data_ptr())
        torch.cuda.synchronize()
        same(tuple(t.cpu().numpy() for t in (di, ds, dp)), host["search_probed"], "search_probed_device")
    if m.codes:
        di, ds, dc, do = outs(rd.cq, (rd.ck, i64), (rd.ck, f32), (rd.refine, i64), (rd.refine, f32))
        ix.search_coded_device(dq.data_ptr(), rd.cq, rd.ck, di.data_ptr(), ds.data_ptr(), rd.refine, SCALE, 0.0, s,
                               d_cand=dc.data_ptr(), d_coarse=do.data_ptr())
        torch.cuda.synchronize()
        same(tuple(t.cpu().numpy() for t in (di, ds, dc, do)), host["search_coded"], "search_coded_device")


def check(ix, m, rd, device=False, what=""):
    q = queries()
    # 1. the model
    assert len(ix) == m.size and ix.live == m.live and ix.dtype == m.dt, what
    assert np.array_equal(ix.is_live(), m.is_live()), what
    assert ix.has_codes == m.codes and ix.n_lists == m.n_lists, what
    if m.size:
        bits_equal_with_nans(ix.rows(), m.rows())
        if m.codes:
            got, want = ix.codes(), codes_oracle(m.rows())
            assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1])), what
    # 2. the anchor
    thr = 0.0
    if m.size:
        L = logits(q[:5], m.rows())
        thr = threshold_between(L, m.is_live(), 40)
        if not m.has_nan():
            assert_same(ix.search(q[:5], 10, SCALE), logits_oracle(L, m.is_live(), 10), what)
    # 3. a fresh handle
    host = {}
    with fresh(m) as f:
        for name, step in check_reads(rd).items():
            host[name] = read(ix, step, thr)
            kind = "no partition" if name == "lists" and m.part != "current" else m.refusal(step[0])
            if kind:  # the message is the model's; the fresh handle has no stale partition to speak of
                assert host[name][0] == "refused" and cases.REFUSALS[kind] in host[name][1], (what, name, host[name])
                continue
            same(host[name], read(f, step, thr), (what, name))
            if name != "kmeans":  # which a NaN in the gallery refuses, on both handles
                assert host[name] == () or not isinstance(host[name][0], str), (what, name, host[name])
    if device and m.size:
        device_forms(ix, m, rd, host)


def read_step(ix, m, step, what):
    """A read step of a script: against the oracle where the step names one, else against a fresh handle."""
    from open_clip_inference.error import ResultOverflow
    op, kind = step[0], m.refusal(step[0])
    if kind:
        got = read(ix, step, 0.0)
        assert got[0] == "refused" and cases.REFUSALS[kind] in got[1], (what, got[:2])
        return
    if op == "range_search":
        nq, mode = step[1], step[2]
        q, ok = queries()[:nq], m.is_live()
        L = logits(q, m.rows())
        thr = threshold_between(L, ok, 3) if mode == "three" else 10.0
        want = range_oracle(L, thr, ok)
        total = int(want[0][-1])
        if mode == "three" and ok.sum() * nq >= 4 and not m.has_nan():
            assert total == 3, what
        if mode == "overflow8" and total > 8:
            with pytest.raises(ResultOverflow) as e:
                ix.range_search(q, thr, SCALE, max_results=8)
            assert e.value.needed == total, what
        else:
            assert_range(ix.range_search(q, thr, SCALE, max_results=max(total, 1)), want, what)
        return
    with fresh(m) as f:
        same(read(ix, step), read(f, step), what)


def run_script(script, capacity, dt, rd):
    from open_clip_inference import EmbeddingIndex
    from open_clip_inference.error import ClipError
    m = Model(cases.E, capacity, dt)
    with EmbeddingIndex(cases.E, capacity, dtype=dt) as ix:
        for at, step in enumerate(script):
            what = f"step {at}: {step[:2]}"
            if step[0] == "check":
                check(ix, m, rd, device=len(step) > 1, what=what)
            elif step[0] in cases.MUTATIONS:
                try:
                    m.apply(step)
                except Refused as e:
                    with pytest.raises(ClipError, match=cases.REFUSALS[e.kind]):
                        mutate(ix, step)
                    continue
                mutate(ix, step)
            else:
                read_step(ix, m, step, what)


# ---- the tests --------------------------------------------------------------------------------------------
def test_two_fresh_handles_agree():
    """Comparison 3 rests on this: two fresh handles of equal state return the same bits from every read form,
    the probabilities and their (max, sum) rows included."""
    m = Model(cases.E, cases.CAPACITY, "f32")
    for step in (("add", 500, 21), ("remove", cases.ids(3, 64, 499)), ("enable_codes",), ("partition", 17, 5),
                 ("remove", cases.ids(100))):
        m.apply(step)
    for rd in (READS, SMALL_READS):
        with fresh(m) as a, fresh(m) as b:
            L = logits(queries()[:5], m.rows())
            thr = threshold_between(L, m.is_live(), 40)
            for name, step in check_reads(rd).items():
                ra, rb = read(a, step, thr), read(b, step, thr)
                assert not isinstance(ra[0], str), (name, ra)
                same(ra, rb, name)
            check(a, m, rd, device=True, what="a fresh handle against the model")


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_one_handle_through_the_script(dt):
    run_script(cases.SCRIPT, cases.CAPACITY, dt, READS)


@pytest.mark.parametrize("seed", [1, 2])
def test_one_handle_through_a_random_script(seed):
    run_script(cases.random_script(seed, 40), cases.CAPACITY, "f32", READS)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_many_queries_on_a_tiny_handle(dt):
    """Capacity 20, read with 260 queries and k = refine = nprobe = 128: the workspace is sized from the capacity,
    the query chunk is 256 whatever the capacity."""
    run_script(cases.SMALL_SCRIPT, cases.SMALL_CAPACITY, dt, SMALL_READS)
