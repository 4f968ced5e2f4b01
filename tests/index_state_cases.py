"""A numpy model of an EmbeddingIndex handle's state and the scripts that tests/test_gpu_index_state.py runs on
one long-lived handle (tests/test_cpu_index_state.py checks both on the CPU).

  Model          what the mutating operations leave behind: the rows as stored, the size, the live flags, codes
                 on or off, the partition's state and centroids; and which calls are refused.  It knows nothing
                 of searching: what a search returns comes from the oracles of the per-feature suites.
  SCRIPT         one hand-written list of steps that takes every lazily grown buffer of the handle both ways
                 (small then large: reallocated; large then small: kept, and nothing of the larger call may be
                 read) and holds the sequences in which host state has gone wrong before.
  SMALL_SCRIPT   a short script for a handle of capacity 20 read with 260 queries, k = refine = nprobe = 128.
  random_script  the same operations drawn at random, with valid and now and then invalid arguments.

A step is a tuple (op, args...); rows and centroids are named by a seed (rows_for, centroids_for), ids are
given outright.  ("check",) compares the whole handle; ("check", "device") uses the device forms as well.
No GPU import."""
import numpy as np

from tests.index_cases import ROUND, unit_rows

E = 80           # a short last slab; code rows are padded to 128
CAPACITY = 600   # more than two query chunks of a self-join, several 64-row spans
SMALL_CAPACITY = 20
SMALL_READS = dict(nq=260, k=128, refine=128, nprobe=128)

MUTATIONS = ("add", "add_device", "remove", "set_rows", "clear", "enable_codes", "drop_codes", "partition",
             "drop_partition")
READS = ("search", "search_probs", "range_search", "duplicates", "assign", "kmeans", "rows", "rows_at",
         "search_probed", "search_coded")
# kind -> a piece of the library's message for it
REFUSALS = {"full": "index full", "bad id": "id out of range", "duplicate id": "duplicate id",
            "no partition": "partition", "no codes": "no codes", "empty": "Empty batch"}


class Refused(Exception):
    def __init__(self, kind):
        super().__init__(kind)
        self.kind = kind


def rows_for(seed, n, E=E, nan=False):
    """n unit rows [n][E] named by `seed`; nan: the first element of the first row is a NaN."""
    x = unit_rows(np.random.default_rng(50021 + seed), n, E)
    if nan:
        x[0, 0] = np.nan
    return x


def centroids_for(seed, C, E=E):
    return unit_rows(np.random.default_rng(90001 + seed), C, E)


class Model:
    def __init__(self, E, capacity, dt="f32"):
        self.E, self.capacity, self.dt = E, capacity, dt
        self.stored = np.zeros((capacity, E), np.float32)
        self.size = 0
        self.alive = np.ones(capacity, bool)  # flags at and past `size` are True
        self.codes = False
        self.part = "none"  # none | current | stale
        self.cen = None
        self.part_alive = None  # the live flags when the partition was made

    # ---- what the handle reports --------------------------------------------------------------------------
    def rows(self):
        return self.stored[:self.size]

    def is_live(self):
        return self.alive[:self.size].copy()

    @property
    def live(self):
        return int(self.alive[:self.size].sum())

    @property
    def n_lists(self):
        return {"none": 0, "stale": -1, "current": 0 if self.cen is None else len(self.cen)}[self.part]

    def has_nan(self):
        return bool(np.isnan(self.rows()).any())

    def _round(self, x):
        x = np.ascontiguousarray(x, np.float32)
        return x.copy() if self.dt == "f32" else ROUND[self.dt](x)

    def _stale(self):
        if self.part != "none":
            self.part = "stale"

    def _check_ids(self, ids, unique):
        ids = np.asarray(ids, np.int64)
        if ((ids < 0) | (ids >= self.size)).any():
            raise Refused("bad id")
        if unique and len(np.unique(ids)) != len(ids):
            raise Refused("duplicate id")
        return ids

    # ---- the mutating operations; a refusal changes nothing -----------------------------------------------
    def add(self, rows):
        n = len(rows)
        if n > self.capacity - self.size:
            raise Refused("full")
        self.stored[self.size:self.size + n] = self._round(rows)
        self.size += n
        self._stale()

    add_device = add

    def remove(self, ids):
        ids = self._check_ids(ids, unique=False)
        self.alive[ids] = False  # the partition stays current: the live flag rejects the row

    def set_rows(self, ids, rows):
        ids = self._check_ids(ids, unique=True)
        if len(ids) == 0:
            return
        self.stored[ids] = self._round(rows)
        self.alive[ids] = True
        self._stale()

    def clear(self):
        self.size = 0
        self.alive[:] = True
        self._stale()

    def enable_codes(self):
        self.codes = True

    def drop_codes(self):
        self.codes = False

    def partition(self, cen):
        if self.size == 0:
            raise Refused("empty")
        self.part, self.cen = "current", np.ascontiguousarray(cen, np.float32).copy()
        self.part_alive = self.alive.copy()  # a row removed later stays in its list

    def drop_partition(self):
        self.part, self.cen = "none", None

    # ---- the read forms: only whether they are refused ----------------------------------------------------
    def refusal(self, op):
        """The kind of refusal of read form `op` in this state, or None."""
        if op == "search_probed" and self.part != "current":
            return "no partition"
        if op == "search_coded" and not self.codes:
            return "no codes"
        if self.size == 0 and op in READS and op not in ("rows", "rows_at"):
            return "empty"
        return None

    def apply(self, step):
        """Applies a mutating step of a script; raises Refused as the handle would."""
        op, args = step[0], step[1:]
        if op in ("add", "add_device"):
            n, seed = args[0], args[1]
            getattr(self, op)(rows_for(seed, n, self.E, nan=len(args) > 2))
        elif op == "set_rows":
            ids, seed = args[0], args[1]
            self.set_rows(ids, rows_for(seed, len(ids), self.E, nan=len(args) > 2))
        elif op == "remove":
            self.remove(args[0])
        elif op == "partition":
            self.partition(centroids_for(args[1], args[0], self.E))
        else:
            getattr(self, op)()


def ids(*a):
    return tuple(int(i) for i in np.r_[a])


CHECK, DEVICE_CHECK = ("check",), ("check", "device")

SCRIPT = [
    # codes enabled on an empty handle, then rows; every read of an empty gallery is refused
    CHECK,
    ("enable_codes",), CHECK,
    ("add", 3, 1), CHECK,                       # a 16-bit add of 3 rows: the scratch is allocated small
    ("set_rows", ids(1), 2), CHECK,             # set_rows of 1 row
    ("add", 97, 3),                             # size 100
    ("assign", 3, 1), ("assign", 65, 2), ("assign", 3, 1),     # rows 100; C 3, 65, 3
    ("kmeans", 4, 1), ("kmeans", 17, 2), ("kmeans", 4, 1),
    ("range_search", 5, "overflow8"), ("range_search", 5, "exact"), ("range_search", 5, "three"),
    ("partition", 65, 1), ("search_probed", 5, 10, 65), ("search_probed", 5, 10, 1), CHECK,
    ("partition", 3, 2), ("search_probed", 260, 128, 2), ("search_probed", 1, 1, 2), CHECK,
    ("add", 300, 4), ("rows",), CHECK,          # a 16-bit add of 300 rows: the scratch grows; stale partition
    ("search_probed", 5, 10, 2),                # refused: stale; the handle stays usable
    ("partition", 3, 2), CHECK,                 # again after more rows were added (pt_ids grows, pt_off does not)
    ("add_device", 100, 5), DEVICE_CHECK,       # add_device beside add; size 500
    ("assign", 3, 1), ("assign", 65, 2),        # rows 500: the label buffers grow
    ("kmeans", 17, 2), ("kmeans", 4, 1),
    ("set_rows", ids(np.arange(300) * 5 // 3), 6), CHECK,     # set_rows of 300
    ("set_rows", ids(499), 7), ("rows_at", 400), ("rows_at", 2), CHECK,
    ("search", 260, 128), ("search", 1, 1), ("search", 260, 1), ("search", 1, 128),
    ("search_probs", 260, 128), ("search_probs", 1, 1),
    ("search_coded", 260, 128, 128), ("search_coded", 1, 1, 16), ("search_coded", 5, 16, 128),
    ("search_coded", 5, 16, 16),
    ("partition", 65, 1), ("search_probed", 260, 128, 65), ("search_probed", 1, 1, 1), CHECK,
    ("remove", ids(7, 64, 65, 499)), CHECK,     # still current
    ("search_probed", 5, 10, 2),
    ("add", 90, 8), CHECK,                      # remove, add: the new rows are live; the partition is stale
    ("add", 11, 9), CHECK,                      # a refused add past capacity (590 + 11) between two checks
    ("remove", ids(589)), ("clear",), ("add", 40, 10), ("remove", ids(3)), CHECK,   # fewer rows after a clear
    ("search_coded", 5, 10, 32),                # the codes behind row 40 are those of the earlier gallery
    ("assign", 3, 1), ("kmeans", 4, 1), ("range_search", 5, "three"), ("duplicates",),
    ("partition", 3, 2), DEVICE_CHECK,
    ("drop_codes",), CHECK,
    ("search_coded", 5, 10, 32),                # refused: no codes
    ("set_rows", ids(0, 3, 39), 11), ("add_device", 25, 12), ("remove", ids(41, 42)),
    ("enable_codes",), CHECK,                   # codes dropped, mutations, codes again
    ("partition", 3, 2),
    ("remove", ids(np.arange(65))), CHECK,      # every row removed: every search pads
    ("search", 5, 10), ("search_probs", 5, 10), ("search_coded", 5, 10, 32), ("range_search", 5, "three"),
    ("search_probed", 5, 10, 2), ("duplicates",), ("assign", 3, 1), ("kmeans", 4, 1),
    ("set_rows", ids(2, 64), 13), CHECK,        # two rows revived
    ("remove", ids(65)), CHECK, ("set_rows", ids(1, 1), 14), CHECK,   # refused: a bad id, a duplicate id
    ("set_rows", ids(5), 15, "nan"), CHECK,     # a NaN in the gallery
    ("drop_partition",), CHECK,
    ("search_probed", 5, 10, 2),                # refused: no partition
    ("clear",), CHECK,
    ("add", 600, 16), ("partition", 3, 3), DEVICE_CHECK,
]

SMALL_SCRIPT = [
    ("add", 12, 1), CHECK,
    ("enable_codes",), ("partition", 5, 1), DEVICE_CHECK,
    ("remove", ids(0, 11)), CHECK,
    ("add_device", 8, 2), CHECK,
    ("add", 1, 3), CHECK,                       # refused
    ("partition", 20, 2), ("set_rows", ids(0, 19), 4), ("partition", 2, 3), CHECK,
    ("clear",), ("add", 1, 5), ("partition", 1, 1), CHECK,
]


def random_script(seed, steps, E=E, capacity=CAPACITY):
    """`steps` operations drawn from the mutations and the read forms, a check after about half of them and at
    the end; about one argument in eight is invalid (an add past capacity, an id at `size`, a repeated id)."""
    rng = np.random.default_rng(seed)
    m = Model(E, capacity)
    out = [("add", int(rng.integers(1, 200)), int(rng.integers(1 << 20)))]
    m.apply(out[0])
    ops = MUTATIONS + READS
    weight = np.array([4, 3, 4, 4, 1, 2, 1, 3, 1] + [1] * len(READS), float)
    while len(out) < steps:
        op = ops[rng.choice(len(ops), p=weight / weight.sum())]
        bad = rng.integers(8) == 0
        s = int(rng.integers(1 << 20))
        room = capacity - m.size
        if op in ("add", "add_device"):
            if room == 0 and not bad:
                continue
            step = (op, room + 1 if bad else int(rng.integers(1, min(room, 150) + 1)), s)
        elif op in ("remove", "set_rows"):
            if m.size == 0:
                continue
            n = int(rng.integers(1, min(m.size, 70) + 1))
            chosen = rng.choice(m.size, n, replace=False).tolist()
            if bad:
                chosen[int(rng.integers(n))] = m.size if (op == "remove" or rng.integers(2) or n == 1) else chosen[-1]
            step = (op, ids(chosen)) if op == "remove" else (op, ids(chosen), s)
        elif op == "partition":
            step = (op, int(rng.choice([1, 3, 17, 65])), s)
        elif op in MUTATIONS:
            step = (op,)
        else:
            nq, k = int(rng.choice([1, 5, 17, 260])), int(rng.choice([1, 10, 128]))
            step = {"search": (op, nq, k), "search_probs": (op, nq, k),
                    "search_probed": (op, nq, k, int(rng.choice([1, 2, 65]))),
                    "search_coded": (op, nq, k, int(rng.choice([k, 128]))),
                    "range_search": (op, 5, str(rng.choice(["overflow8", "exact", "three"]))),
                    "duplicates": (op,), "assign": (op, int(rng.choice([3, 65])), s),
                    "kmeans": (op, int(rng.choice([4, 17])), s), "rows": (op,),
                    "rows_at": (op, int(rng.integers(1, 50)))}[op]
        out.append(step)
        if op in MUTATIONS:
            try:
                m.apply(step)
            except Refused:
                pass
            if rng.integers(2):
                out.append(CHECK)
    out.append(DEVICE_CHECK)
    return out


# ---- what a script covers, derived by walking it with the model ------------------------------------------
GROW_PAIRS = ("set_rows n", "add n", "range max_results", "assign rows", "assign C", "kmeans C", "partition C",
              "partition rows", "queries", "k", "refine", "nprobe")


def walk(script, E=E, capacity=CAPACITY):
    """(metrics, refusals, ops, checked): per name of GROW_PAIRS the sizes the script asks for, in order; the
    kinds of refusal it meets; the operations it holds; the mutations ("<op>", or "<op> refused") that a check
    follows with no other mutation in between."""
    m = Model(E, capacity)
    metrics = {name: [] for name in GROW_PAIRS}
    refusals, ops, checked, last = set(), set(), set(), None
    for step in script:
        op = step[0]
        ops.add(op)
        if op == "check":
            if last:
                checked.add(last)
            last = None
            for r in READS:
                if m.refusal(r):
                    refusals.add(m.refusal(r))
            continue
        if op in MUTATIONS:
            try:
                m.apply(step)
            except Refused as e:
                refusals.add(e.kind)
                last = op + " refused"
                continue
            last = op
            if op == "set_rows":
                metrics["set_rows n"].append(len(step[1]))
            elif op == "add":
                metrics["add n"].append(step[1])
            elif op == "partition":
                metrics["partition C"].append(step[1])
                metrics["partition rows"].append(m.size)
            continue
        kind = m.refusal(op)
        if kind:
            refusals.add(kind)
            continue
        if op in ("search", "search_probs", "search_probed", "search_coded"):
            metrics["queries"].append(step[1])
            metrics["k"].append(step[2])
        if op == "search_probed":
            metrics["nprobe"].append(step[3])
        elif op == "search_coded":
            metrics["refine"].append(step[3])
        elif op == "range_search":  # 8 < the total of the fixed threshold (hundreds) > 3
            metrics["range max_results"].append({"overflow8": 8, "exact": 1000, "three": 3}[step[2]])
            if step[2] == "overflow8":
                refusals.add("overflow")
        elif op == "assign":
            metrics["assign rows"].append(m.size)
            metrics["assign C"].append(step[1])
        elif op == "kmeans":
            metrics["kmeans C"].append(step[1])
    return metrics, refusals, ops, checked


def goes_both_ways(v):
    """True if the sequence holds a later larger and a later smaller value."""
    up = any(a < b for i, a in enumerate(v) for b in v[i + 1:])
    down = any(a > b for i, a in enumerate(v) for b in v[i + 1:])
    return up and down
