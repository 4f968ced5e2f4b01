"""Cross-stream order of the embedding index, proven with a dependency that is still pending when the dependent
call is made.

One handle owns one workspace, one filter area, one pair area, the coarse and code work areas and the gallery.
What keeps operations on different streams apart is one event: device forms wait for it on their stream and record
it again, host forms synchronise on it.  The older "add on one stream, search on another" tests put nothing in
front of the first operation, so it has finished long before the second is called, ordered or not.  Here every
case puts a clock-probe delay (clipgpu_test_clock_probe) on stream s1 in front of operation A, calls B while the
delay still runs (`pending`, asserted), and then compares results bit for bit with the existing oracles:

  write, then read   A = add_device(G2[64:]) on s1 over a gallery whose rows 64.. physically hold G1 (and, with
                     codes, the codes of G1).  B, a device form on s2 or a host form, must see G2.
  read, then write   A = a device read form over G1 on s1; then something overwrites what it reads (clear + add,
                     set_rows, remove, drop_codes, partition).  A's outputs must be the G1 results.
  close              A = search_device; close() returns after A, with the outputs complete.

Every case first computes, on the CPU, what the result would be had the operation seen the other state, and
asserts that it differs from the expected one: a case that cannot fail is an error in the test.  The two
drop_codes cases are the exception (the other state has no codes to search, or equal ones): they bite through
the assertion that the host call returned only after A had finished.  One control shows that the harness does see
an unordered dependency: a copy into the query buffer, which involves no index operation and which the handle
does not promise to order.

Every stale read or early write these cases are built to catch stays inside memory the handle allocated at its
creation; a case that fails here fails by comparison.  There are no timing assertions: `pending` and the probe's
tick count are conditions of the test.

Out of scope: two device searches that overlap in time on the shared workspace.  With a delay in front, the
unordered one simply finishes first and both are right; seeing it would take real overlap, which is luck."""
import functools

import numpy as np
import pytest

from tests import index_cluster_cases as cluster
from tests import index_codes_cases as codes
from tests import index_ivf_cases as ivf
from tests import index_probs_cases as probs
from tests.index_cases import ROUND, logits_oracle, pattern, unit_rows
from tests.index_range_cases import join_oracle, range_oracle

pytestmark = pytest.mark.gpu

# The delay in front of A, in microseconds.  A condition of the tests, not a tolerance: B must be called while A
# cannot have run.  Between the delay's launch and the `pending` reading lie the launches of A and B and, for the
# read-then-write cases, one host call that must block.  Those cost well under a millisecond, except the first
# launch from a kernel unit in a process, which loads its code object: at 20 ms (the similarity test uses 3 ms for
# one call) `pending` failed once in five runs on the MI355X, in the first case of the file, and held everywhere
# else.  So the stream-pair fixture warms the search path up, and the delay is five times as long.
D_US = 100000

E, CAP, NQ, K, SCALE = 80, 264, 5, 12, 100.0
REFINE, NPROBE = 32, 2
RANGE_THR, RANGE_CAP = 15.0, 4096   # 1.4 sigma of a logit (sigma = 100 / sqrt(80)): about a hundred records
JOIN_THR = 25.0                     # 2.2 sigma: some hundreds of the 34716 pairs
ROWS_AT = np.array([263, 64, 0, 100, 64], np.int64)
PRE_DEAD = 7                        # removed before the remove cases, so that the live bitmap is in use


@functools.lru_cache(maxsize=None)
def data():
    """(G1, G2, queries, centroids, other centroids): unit rows from different seeds, never written to."""
    out = (unit_rows(np.random.default_rng(101), CAP, E), unit_rows(np.random.default_rng(202), CAP, E),
           unit_rows(np.random.default_rng(303), NQ, E), unit_rows(np.random.default_rng(404), 3, E),
           unit_rows(np.random.default_rng(505), 4, E))
    for a in out:
        a.setflags(write=False)
    return out


def stored(g, dt):
    return np.ascontiguousarray(g) if dt == "f32" else ROUND[dt](g)


def lf_gpu(a, b, scale=SCALE):
    """The logits as the library computes them (similarity, pinned bit for bit in tests/test_gpu_similarity.py)."""
    from open_clip_inference.engine import similarity
    return similarity(np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32), scale, 0.0, "logits", 1)


def lf_cpu(a, b, scale=SCALE):
    """The CPU stand-in of the "must bite" checks."""
    return (np.asarray(a, np.float64) @ np.asarray(b, np.float64).T * scale).astype(np.float32)


class State:
    """What an operation sees: the rows as stored, the live flags and, for a probed search, the partition
    (centroids, the rows and live flags it was made from)."""

    def __init__(self, rows, ok=None, part=None):
        self.rows, self.ok, self.part = rows, np.ones(len(rows), bool) if ok is None else ok, part


def bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def differs(a, b):
    return any(x.shape != y.shape or not np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def assert_bits(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, i, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(bits(g), bits(w)), (what, i)


# ---- the device side: inputs and outputs, made and synchronised before the delay -------------------------
class Dev:
    def __init__(self):
        import torch
        from open_clip_inference.index import pack_allow
        G1, G2, Q, CEN, CEN2 = data()
        up = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731  (a copy: the inputs are read-only)
        self.q, self.cen, self.g2 = up(Q), up(CEN), up(G2)
        self.allow = up(pack_allow(pattern(CAP)).view(np.int32))
        new = lambda shape, t: torch.full(shape, -7, dtype=t, device="cuda")  # noqa: E731
        i64, i32, f32 = torch.int64, torch.int32, torch.float32
        self.idx, self.score, self.prob, self.norm = new((NQ, K), i64), new((NQ, K), f32), new((NQ, K), f32), new((NQ, 2), f32)
        self.rq, self.rr, self.rs, self.rtotal = new((RANGE_CAP,), i32), new((RANGE_CAP,), i32), new((RANGE_CAP,), f32), new((1,), i64)
        self.label, self.lscore = new((CAP,), i32), new((CAP,), f32)
        self.cand, self.coarse, self.probes = new((NQ, REFINE), i64), new((NQ, REFINE), f32), new((NQ, NPROBE), i64)
        torch.cuda.synchronize()

    @staticmethod
    def down(*ts):
        return tuple(t.cpu().numpy() for t in ts)


# ---- the forms: what they return in a given state, and how they are called --------------------------------
class Form:
    codes = partition = False
    allow = None  # bool [CAP] or None

    def __init__(self, name):
        self.name = name

    def ok(self, st):
        return st.ok if self.allow is None else st.ok & self.allow

    def compare(self, got, want, st, what):
        assert_bits(got, want, what)

    def result_rows(self, want):
        """The rows in the result: what a remove takes away."""
        return np.unique(want[0][want[0] >= 0])


class Search(Form):
    def __init__(self, name, allow=False):
        super().__init__(name)
        self.allow = pattern(CAP) if allow else None

    def want(self, lf, st):
        return logits_oracle(lf(data()[2], st.rows), self.ok(st), K)

    def device(self, ix, d, s):
        ix.search_device(d.q.data_ptr(), NQ, K, d.idx.data_ptr(), d.score.data_ptr(), SCALE, 0.0, s,
                         d_allow=0 if self.allow is None else d.allow.data_ptr())

    def collect(self, d):
        return d.down(d.idx, d.score)

    def host(self, ix):
        return ix.search(data()[2], K, SCALE, allow=self.allow)


class Probs(Search):
    """Indices and logits exactly; the probabilities and (max, sum) rows to the derived bound of
    tests/index_probs_cases.py, as tests/test_gpu_index_probs.py holds them."""

    def device(self, ix, d, s):
        ix.search_probs_device(d.q.data_ptr(), NQ, K, d.idx.data_ptr(), d.score.data_ptr(), d.prob.data_ptr(), SCALE,
                               0.0, "softmax", s, d_norm=d.norm.data_ptr())

    def collect(self, d):
        return d.down(d.idx, d.score, d.prob, d.norm)

    def host(self, ix):
        return ix.search_probs(data()[2], K, SCALE, 0.0, "softmax", return_norm=True)

    def compare(self, got, want, st, what):
        assert_bits(got[:2], want, what)
        probs.check(got, lf_gpu(data()[2], st.rows), self.ok(st), what)


class Range(Form):
    def want(self, lf, st):
        return range_oracle(lf(data()[2], st.rows), RANGE_THR, self.ok(st))

    def device(self, ix, d, s):
        ix.range_search_device(d.q.data_ptr(), NQ, RANGE_THR, RANGE_CAP, d.rq.data_ptr(), d.rr.data_ptr(),
                               d.rs.data_ptr(), d.rtotal.data_ptr(), SCALE, 0.0, s)

    def collect(self, d):
        """The records in the host form's order: by query, then descending score, then ascending row."""
        total = int(d.rtotal.cpu()[0])
        assert 0 <= total <= RANGE_CAP
        q, r, s = (a[:total] for a in d.down(d.rq, d.rr, d.rs))
        order = np.lexsort((r, -s, q))
        lims = np.concatenate([[0], np.cumsum(np.bincount(q, minlength=NQ))]).astype(np.int64)
        return lims, r[order].astype(np.int64), s[order]

    def host(self, ix):
        return ix.range_search(data()[2], RANGE_THR, SCALE, max_results=RANGE_CAP)

    def result_rows(self, want):
        return np.unique(want[1])


class Assign(Form):
    def want(self, lf, st):
        return cluster.assign_oracle(lf(data()[3], st.rows), self.ok(st))

    def device(self, ix, d, s):
        ix.assign_device(d.cen.data_ptr(), 3, d.label.data_ptr(), d.lscore.data_ptr(), SCALE, 0.0, s)

    def collect(self, d):
        label, score = d.down(d.label, d.lscore)
        return label.astype(np.int64), score

    def host(self, ix):
        return ix.assign(data()[3], SCALE)

    def result_rows(self, want):
        return np.arange(64)  # every row is in the result: one 64-row block of them


class Coded(Form):
    codes = True

    def want(self, lf, st):
        Q = data()[2]
        (idx, score), cand, coarse = codes.expect(lf(Q, st.rows), st.rows, Q, self.ok(st), K, REFINE)
        return idx, score, cand, coarse

    def device(self, ix, d, s):
        ix.search_coded_device(d.q.data_ptr(), NQ, K, d.idx.data_ptr(), d.score.data_ptr(), REFINE, SCALE, 0.0, s,
                               d_cand=d.cand.data_ptr(), d_coarse=d.coarse.data_ptr())

    def collect(self, d):
        return d.down(d.idx, d.score, d.cand, d.coarse)

    def host(self, ix):
        return ix.search_coded(data()[2], K, REFINE, SCALE, return_candidates=True)


class Probed(Form):
    partition = True

    def want(self, lf, st):
        Q = data()[2]
        cen, prows, pok = st.part
        labels = cluster.assign_oracle(lf(cen, prows, 1.0), pok)[0]
        probes = ivf.probes_oracle(lf(Q, cen, 1.0), NPROBE)
        return ivf.probed_oracle(lf(Q, st.rows), labels, probes, self.ok(st), K) + (probes,)

    def device(self, ix, d, s):
        ix.search_probed_device(d.q.data_ptr(), NQ, K, NPROBE, d.idx.data_ptr(), d.score.data_ptr(), SCALE, 0.0, s,
                                d_probes=d.probes.data_ptr())

    def collect(self, d):
        return d.down(d.idx, d.score, d.probes)


class HostOnly(Form):
    """A host form given as (want(lf, st), call(ix))."""

    def __init__(self, name, want, call, codes=False):
        super().__init__(name)
        self.want, self.host, self.codes = want, call, codes


def want_kmeans(lf, st):
    r = cluster.lloyd(st.rows, data()[4], 2, st.ok, logits_fn=lambda c, g: lf(c, g, 1.0))
    return r["centroids"], r["labels"], r["scores"], r["counts"], r["moved"], np.int64(r["iters"])


def call_kmeans(ix):
    km = ix.kmeans(init=data()[4], max_iter=2)
    return km.centroids, km.labels, km.scores, km.counts, km.moved, np.int64(km.iters)


def want_lists(lf, st):
    return ivf.lists_oracle(cluster.assign_oracle(lf(data()[3], st.rows, 1.0), st.ok)[0], 3)


def call_lists(ix):
    ix.partition(data()[3])
    return ix.lists()


def call_enable_codes(ix):
    ix.enable_codes()
    return ix.codes()


DEVICE_READS = [Search("search_device"), Search("search_device d_allow", allow=True), Probs("search_probs_device"),
                Range("range_search_device"), Assign("assign_device"), Coded("search_coded_device")]
HOST_READS = [
    Search("search"), Probs("search_probs"), Range("range_search"),
    HostOnly("duplicates", lambda lf, st: join_oracle(lf(st.rows, st.rows), JOIN_THR, st.ok),
             lambda ix: ix.duplicates(JOIN_THR, SCALE, max_pairs=RANGE_CAP)),
    Assign("assign"), HostOnly("kmeans", want_kmeans, call_kmeans),
    HostOnly("rows(64, 200)", lambda lf, st: (st.rows[64:264],), lambda ix: (ix.rows(64, 200),)),
    HostOnly("rows_at", lambda lf, st: (st.rows[ROWS_AT],), lambda ix: (ix.rows_at(ROWS_AT),)),
    HostOnly("codes(64, 200)", lambda lf, st: codes.codes_oracle(st.rows[64:264]), lambda ix: ix.codes(64, 200), codes=True),
    HostOnly("enable_codes, codes()", lambda lf, st: codes.codes_oracle(st.rows), call_enable_codes),
    HostOnly("partition, lists()", want_lists, call_lists),
    Coded("search_coded"),
]
READ_FORMS = DEVICE_READS[:5] + [Probed("search_probed_device"), DEVICE_READS[5]]
OVERWRITES = ["clear, add_device on s2", "clear, add", "set_rows", "remove"]
READ_WRITE = [(f, o, "f32") for f in READ_FORMS for o in OVERWRITES]
READ_WRITE += [(f, OVERWRITES[0], "bf16") for f in READ_FORMS]
READ_WRITE += [(READ_FORMS[6], o, "f32") for o in ("drop_codes", "drop_codes, enable_codes")]
READ_WRITE += [(READ_FORMS[5], "partition(other centroids)", "f32")]


# ---- the harness ------------------------------------------------------------------------------------------
D2_US = 2000  # the marker in front of B on s2: long enough to be still running when B is launched


class NotSideBySide(Exception):
    """s2 waited behind the delay on s1: the attempt proves nothing."""


def delay(stream, probe, us=D_US):
    from open_clip_inference import _lib
    _lib.check(_lib.lib().clipgpu_test_clock_probe(stream.cuda_stream, us, probe.data_ptr()))


def warm_up(stream):
    """The first launches of the process, which load code objects, happen here and not behind a delay."""
    import torch
    from open_clip_inference import EmbeddingIndex
    Q = data()[2]
    d = Dev()
    for dt in ("f32", "bf16"):
        with EmbeddingIndex(E, CAP, dtype=dt) as ix:
            ix.add_device(d.g2.data_ptr(), CAP, stream.cuda_stream)
            ix.search_device(d.q.data_ptr(), NQ, K, d.idx.data_ptr(), d.score.data_ptr(), SCALE, 0.0, stream.cuda_stream)
            ix.search(Q, K, SCALE)
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def pair():
    """(s1, candidates for s2).  A process has a few hardware queues and two streams may share one, in which case
    work on the second waits behind the delay on the first and every order test would pass whatever the library
    does.  Control: the delay on s1, a tiny fill on s2; s2 must finish while s1 has not.  At least one of 8
    candidates must pass it here, or the fixture fails: a skipped order suite is no order suite.  Which streams
    share a queue can change while the process runs, so every case that puts B on s2 checks again for itself
    (run) and moves on to the next candidate when its s2 did wait (side_by_side)."""
    import torch
    s1 = torch.cuda.Stream()
    probe, t = torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros(16, device="cuda")
    candidates = [torch.cuda.Stream() for _ in range(8)]
    for i, s2 in enumerate(candidates):
        torch.cuda.synchronize()
        delay(s1, probe)
        with torch.cuda.stream(s2):
            t.fill_(1.0)
        s2.synchronize()
        ok = not s1.query()
        s1.synchronize()
        if ok:
            warm_up(s2)
            return s1, candidates[i:] + candidates[:i]
    pytest.fail("no pair of streams runs side by side: 8 candidates all waited behind the delay on the first; "
                "the order tests cannot be trusted without one")


def side_by_side(pair, case):
    """Runs case((s1, s2)), which builds its handle anew and calls run, with the candidates for s2 in turn until
    one did not wait behind the delay; none of 8: the test fails."""
    s1, candidates = pair
    for _ in range(8):
        try:
            return case((s1, candidates[0]))
        except NotSideBySide:
            print("the second stream waited behind the delay on the first: next candidate")
            candidates.append(candidates.pop(0))
    pytest.fail("in 8 attempts the second stream always waited behind the delay on the first")


def run(streams, A, B, host_b):
    """The delay and A on s1, then B (a host call, or a device form on s2) while A cannot yet have run.  In front
    of a device form, s2 gets a short delay of its own and an event: the event must complete while s1 is still
    pending, which shows that s2, busy when B was launched, did not wait behind s1 (else NotSideBySide)."""
    import torch
    s1, s2 = streams
    probe, probe2 = (torch.zeros(2, dtype=torch.int64, device="cuda") for _ in range(2))
    marker = torch.cuda.Event()
    torch.cuda.synchronize()
    delay(s1, probe)
    A(s1.cuda_stream)
    if host_b:
        pending = side = not s1.query()
        out = B(s2.cuda_stream)
    else:
        delay(s2, probe2, D2_US)
        marker.record(s2)
        out = B(s2.cuda_stream)
        pending = not s1.query()
        marker.synchronize()
        side = not s1.query()
    s1.synchronize()
    s2.synchronize()
    assert pending, "B was not called while A was pending: raise D_US"
    assert int(probe[1]) >= D_US * 100, "the delay did not run its time (100 MHz ticks)"
    if not side:
        raise NotSideBySide()
    return out


def index(dt, form, rows):
    from open_clip_inference import EmbeddingIndex
    ix = EmbeddingIndex(E, CAP, dtype=dt)
    if form.codes:
        ix.enable_codes()
    ix.add(rows)
    return ix


# ---- write, then read -------------------------------------------------------------------------------------
def write_then_read(pair, form, dt, host_b):
    G1, G2 = data()[:2]
    seen = State(stored(G2, dt))
    stale = State(np.concatenate([stored(G2[:64], dt), stored(G1[64:], dt)]))
    assert differs(form.want(lf_cpu, seen), form.want(lf_cpu, stale)), "the case cannot fail"
    want = form.want(lf_gpu, seen)

    def case(streams):
        with index(dt, form, G1) as ix:
            ix.clear()
            ix.add(G2[:64])
            d = Dev()
            rest = d.g2[64:]
            assert rest.data_ptr() % 16 == 0

            def B(s):
                if host_b:
                    return form.host(ix)
                form.device(ix, d, s)
            got = run(streams, lambda s: ix.add_device(rest.data_ptr(), CAP - 64, s), B, host_b)
            form.compare(got if host_b else form.collect(d), want, seen, form.name)
            assert len(ix) == CAP
    side_by_side(pair, case)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("form", DEVICE_READS, ids=lambda f: f.name)
def test_a_device_read_on_another_stream_sees_the_rows_of_a_pending_add_device(pair, form, dt):
    write_then_read(pair, form, dt, host_b=False)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("form", HOST_READS, ids=lambda f: f.name)
def test_a_host_read_sees_the_rows_of_a_pending_add_device(pair, form, dt):
    write_then_read(pair, form, dt, host_b=True)


# ---- read, then write -------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,overwrite,dt", READ_WRITE, ids=lambda v: getattr(v, "name", v))
def test_a_pending_device_read_keeps_its_state_when_the_handle_is_written(pair, form, overwrite, dt):
    import torch
    G1, G2, Q, CEN, CEN2 = data()
    s1 = pair[0]
    ok = np.ones(CAP, bool)
    if overwrite == "remove":
        ok[PRE_DEAD] = False
    part = (CEN, stored(G1, dt), ok.copy()) if form.partition else None
    seen = State(stored(G1, dt), ok, part)
    want = form.want(lf_gpu, seen)
    gone = form.result_rows(want)
    other = {"remove": lambda: State(seen.rows, ok & ~np.isin(np.arange(CAP), gone), part),
             "partition(other centroids)": lambda: State(seen.rows, ok, (CEN2, seen.rows, ok))}.get(
                 overwrite, lambda: State(stored(G2, dt), None, part))()
    by_blocking = overwrite.startswith("drop_codes")  # the other state has no codes, or equal ones
    if not by_blocking:
        assert differs(form.want(lf_cpu, seen), form.want(lf_cpu, other)), "the case cannot fail"
    host_b = overwrite != OVERWRITES[0]

    def case(streams):
        with index(dt, form, G1) as ix:
            if overwrite == "remove":
                ix.remove([PRE_DEAD])
            if form.partition:
                ix.partition(CEN)
            d = Dev()

            def B(s):
                if overwrite == "clear, add_device on s2":
                    ix.clear()
                    ix.add_device(d.g2.data_ptr(), CAP, s)
                    return True
                if overwrite == "clear, add":
                    ix.clear()
                    ix.add(G2)
                elif overwrite == "set_rows":
                    ix.set_rows(np.arange(CAP), G2)
                elif overwrite == "remove":
                    ix.remove(gone)
                elif overwrite == "partition(other centroids)":
                    ix.partition(CEN2)
                else:
                    ix.drop_codes()
                    if overwrite.endswith("enable_codes"):
                        ix.enable_codes()
                return s1.query()  # every host write waits for A: it returns only after s1 has run dry
            waited = run(streams, lambda s: form.device(ix, d, s), B, host_b)
            form.compare(form.collect(d), want, seen, (form.name, overwrite))
            assert waited, "the host write returned while A was still pending"
            # the write itself took effect
            if overwrite == "remove":
                assert np.array_equal(ix.is_live(), other.ok) and ix.live == int(other.ok.sum())
            elif overwrite in OVERWRITES[:3]:
                torch.cuda.synchronize()
                assert np.array_equal(bits(ix.rows()), bits(stored(G2, dt))) and ix.live == CAP
    side_by_side(pair, case)


# ---- close ------------------------------------------------------------------------------------------------
def test_close_returns_after_a_pending_search_with_its_outputs_complete(pair):
    G1 = data()[0]
    form = DEVICE_READS[0]
    seen = State(stored(G1, "f32"))
    want = form.want(lf_gpu, seen)
    assert differs(want, (np.full((NQ, K), -7, np.int64), np.full((NQ, K), -7, np.float32)))

    def case(streams):
        ix = index("f32", form, G1)
        d = Dev()

        def B(s):
            ix.close()
            return streams[0].query()
        done = run(streams, lambda s: form.device(ix, d, s), B, True)
        form.compare(form.collect(d), want, seen, "close")
        assert done, "close returned while the search was still pending"
    side_by_side(pair, case)


# ---- the control: the harness sees an unordered dependency -------------------------------------------------
def test_the_harness_sees_a_dependency_the_handle_does_not_order(pair):
    """The query buffer holds NaN; s1 carries the delay and then the copy of the real queries into it; s2 carries
    search_device of that buffer.  No index operation is on s1, so nothing orders the search behind the copy: it
    must return the result of the NaN queries, not of the real ones."""
    import torch
    G1, _, Q = data()[:3]
    form = DEVICE_READS[0]
    real = form.want(lf_gpu, State(G1))
    nanq = logits_oracle(lf_gpu(np.full_like(Q, np.nan), G1), np.ones(CAP, bool), K)
    assert np.isnan(nanq[1]).all() and not np.isnan(real[1]).any()

    def case(streams):
        with index("f32", form, G1) as ix:
            d = Dev()
            real_q = d.q.clone()
            d.q.fill_(float("nan"))
            torch.cuda.synchronize()

            def A(s):
                with torch.cuda.stream(streams[0]):
                    d.q.copy_(real_q, non_blocking=True)
            run(streams, A, lambda s: form.device(ix, d, s), False)  # NotSideBySide if s2 waited behind s1
            idx, score = form.collect(d)
            assert np.isnan(score).all(), "the search ran side by side with s1 and yet behind the copy on it"
            assert np.array_equal(idx, nanq[0])
            assert np.array_equal(d.q.cpu().numpy(), Q)  # the copy did run, afterwards
    side_by_side(pair, case)
