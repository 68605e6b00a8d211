"""Scenes that put chosen list lengths and chosen depth bit patterns into chosen lists, and a numpy model of the path the list
sort takes for each of them (tests/test_sort_scenes_cpu.py, tests/test_gpu_sort.py).

Two facts carry the construction: a tiny isotropic Gaussian lands in exactly one 16 x 8-pixel list, and under an identity c2w the
device depth is bit for bit pos.z.  So `build` decides the length of every list and the 32 key bits of every entry.

sort_path / instantiation / launches RESTATE constants of csrc/gs_sort.h (DENSE_BUCKET, the <T, E, LOG2B> instantiations, the
bucket shift, the global path at T * E entries) and of gsplat_bin in csrc/gsplat_kernels.hip (the `class0` rule, cap() and the grid
limits 256 / 768 / 4096 / 16384).  A change there is made here too: the tests compare the intended path of every list with this
model, not with the kernels themselves."""
import functools

import numpy as np

from tests import list_scenes, listcheck

LIST_W, LIST_H = listcheck.LIST_W, listcheck.LIST_H
SCALE_RAW = -12.0             # sigma = 6e-6 world units: a fraction of a pixel at every depth and focal length used here
DENSE_BUCKET = 48             # gs_sort.h: a bucket with more entries sends the list to the bitonic network
# gs_sort.h, the four instantiations of sort_list: name -> (T, E, LOG2B)
INST = {"wave": (64, 4, 9), "256": (256, 4, 11), "512": (512, 8, 12), "1024": (1024, 8, 13)}
# every (instantiation, path) pair that exists: the 512-thread kernel sorts in global memory only where class 0 has no launch
COMBINATIONS = {("wave", "A"), ("wave", "B"), ("256", "A"), ("256", "B"), ("512", "A"), ("512", "B"), ("512", "C"),
                ("1024", "A"), ("1024", "B"), ("1024", "C")}
BASE_BITS = 0x3F800000        # 1.0f
NEAR_BITS, FAR_BITS = 0x3F000000, 0x42800000      # 0.5f and 64.0f: inside the default near / far planes (0.01, 100)


# ---- the model of the path choice -------------------------------------------------------------------------------------------
def class0_rule(n_binned, n_lists):
    """gsplat_bin: does the 1024-thread kernel (lists of 4096 entries and more) get a launch of its own?"""
    return n_binned >= 4096 and n_binned >= 256 * n_lists


def instantiation(n, class0):
    """Which instantiation sorts a list of n entries: its name in INST and whether it is a GLOBAL one."""
    if n < 256:
        return "wave", False
    if n < 1024:
        return "256", False
    if n < 4096 or not class0:
        return "512", True
    return "1024", True


def launches(n_binned, n_lists):
    """The grids of gsplat_bin's sort launches as the number of lists each takes per grid-stride pass (0: no launch), by class."""
    def cap(min_len):
        return max(1, min(n_lists, n_binned // min_len))
    c0 = class0_rule(n_binned, n_lists)
    return {"class0": c0,
            "1024": min(cap(4096), 256) if c0 else 0,
            "512": min(cap(1024), 768) if n_binned >= 1024 else 0,
            "256": min(cap(256), 4096) if n_binned >= 256 else 0,
            "wave": 4 * min((cap(1) + 3) // 4, 16384)}


def sort_paths(list_of, depth_bits, class0):
    """The path of every list.  list_of[k] / depth_bits[k]: list and float32 depth bits of pair k.  Returns (lists, length, inst
    name, path, shift) as arrays over the non-empty lists; the shift is the one the kernel computes (unused on path C)."""
    list_of = np.asarray(list_of, np.int64)
    o = np.argsort(list_of, kind="stable")
    ls, bits = list_of[o], np.asarray(depth_bits, np.uint32)[o].astype(np.int64)
    lists, start, n = np.unique(ls, return_index=True, return_counts=True)
    mn, mx = np.minimum.reduceat(bits, start), np.maximum.reduceat(bits, start)
    bl = np.frexp((mx - mn).astype(np.float64))[1]                          # bit length (0 for a range of 0)
    names, glob = zip(*(instantiation(int(x), class0) for x in n))
    names = np.array(names)
    log2b = np.array([INST[x][2] for x in names])
    cap = np.array([INST[x][0] * INST[x][1] for x in names])
    shift = np.maximum(bl - log2b, 0)
    k = np.repeat(np.arange(len(lists)), n)
    bucket = (bits - mn[k]) >> shift[k]
    assert np.all(bucket < (1 << log2b)[k])
    key, cnt = np.unique(k * (1 << 13) + bucket, return_counts=True)
    big = np.zeros(len(lists), np.int64)
    np.maximum.at(big, key >> 13, cnt)
    path = np.where(np.array(glob) & (n >= cap), "C", np.where(big > DENSE_BUCKET, "B", "A"))
    return lists, n, names, path, shift


def sort_path(depth_bits, T, E, LOG2B, global_):
    """The kernel's decision for ONE list sorted by sort_list<T, E, LOG2B, ., global_>: ('A' | 'B' | 'C', shift)."""
    bits = np.asarray(depth_bits, np.uint32).astype(np.int64)
    if global_ and len(bits) >= T * E:
        return "C", 0
    rng_ = int(bits.max() - bits.min())
    shift = max(rng_.bit_length() - LOG2B, 0)
    big = np.bincount((bits - bits.min()) >> shift).max()
    return ("B" if big > DENSE_BUCKET else "A"), shift


# ---- depth patterns: offsets from BASE_BITS, as float32 bit patterns ------------------------------------------------------
def _distinct(rng, n, lo, hi):
    """n distinct integers of [lo, hi], in random order."""
    return lo + rng.permutation(hi - lo + 1)[:n] if hi - lo < 4 * n + 64 else lo + rng.choice(hi - lo + 1, n, replace=False)


def _spread(rng, n, L):
    return BASE_BITS + _distinct(rng, n, 0, 4 * n)


def _equal(rng, n, L):
    return np.full(n, BASE_BITS + 77)


def _clump(rng, n, L, m):
    """m copies of the smallest value (bucket 0); the others distinct over (bucket 0, 8 n], 8 n among them: the range is 8 n, a
    bucket is at most 2^3 bit patterns wide (8 n < 16 x 2^LOG2B), and distinct values put at most 8 entries into each."""
    width = 1 << max((8 * n).bit_length() - L, 0)
    rest = _distinct(rng, n - m - 1, width, 8 * n - 1)
    return BASE_BITS + rng.permutation(np.concatenate([np.zeros(m, np.int64), rest, [8 * n]]))


def _range(rng, n, L, R):
    return BASE_BITS + rng.permutation(np.concatenate([[0, R], _distinct(rng, n - 2, 1, R - 1)]))


def _two_clumps(rng, n, L):
    """Distinct depths, half just above 0.5 and half just above 64: each half falls into one bucket (a bucket is 2^(26 - LOG2B)
    bit patterns wide, a half spans fewer than 2^13), and each half is 49 entries or more."""
    h = n // 2
    return rng.permutation(np.concatenate([NEAR_BITS + _distinct(rng, h, 0, 2 * h), FAR_BITS + _distinct(rng, n - h, 0, 2 * h)]))


def _descending(rng, n, L):
    return np.sort(_spread(rng, n, L))[::-1]


def _range_shift(k):
    return (0, 1, 1, 2)[k]


def pattern(name, rng, n, L):
    """(depth bits [n] in Gaussian-index order, intended LDS path, intended shift or None) of a pattern for sort_list<., ., L>."""
    if name.startswith("range"):
        k = int(name[5:])
        R = ((1 << L) - 1, 1 << L, (1 << (L + 1)) - 1, 1 << (L + 1))[k]
        return _range(rng, n, L, R), "A", _range_shift(k)
    if name.startswith("clump"):
        return _clump(rng, n, L, int(name[5:])), "A" if name == "clump48" else "B", None
    bits = {"spread": _spread, "equal": _equal, "two_clumps": _two_clumps, "descending": _descending}[name](rng, n, L)
    path = {"spread": "A", "equal": "A" if n <= DENSE_BUCKET else "B", "two_clumps": "B", "descending": "A"}[name]
    return bits, path, (0 if name == "equal" else None)


RANGES = ("range0", "range1", "range2", "range3")
ALL_PATTERNS = ("spread", "equal", "clump48", "clump49") + RANGES + ("two_clumps", "descending")


def applies(name, n):
    """Does the pattern exist at length n?  (clumps need other buckets beside them, two_clumps 49 entries in each half)"""
    if name in ("spread", "equal"):
        return True
    if name in ("clump48", "clump49", "two_clumps"):
        return n >= 128
    return n >= 2


# ---- the scene builder ---------------------------------------------------------------------------------------------------
def build(H, W, lists, seed=0, behind=False):
    """lists: {list index: float32 depths of its entries, in the order of their Gaussian indices}.  Returns a scene in the format of
    tests/list_scenes.py (identity c2w, zero SH) whose Gaussians are dealt out to the lists at random, so that the entries of one
    list are spread over the whole index range; s["list_of"] is the list of every Gaussian.  behind: every depth negated (all
    behind the camera, nothing binned)."""
    rng = np.random.default_rng(seed)
    lists_x = (W + LIST_W - 1) // LIST_W
    idx = np.array(sorted(lists), np.int64)
    assert len(idx) and idx[0] >= 0 and idx[-1] < lists_x * ((H + LIST_H - 1) // LIST_H)
    ln = np.array([len(lists[i]) for i in idx])
    list_of = rng.permutation(np.repeat(idx, ln))
    z = np.empty(len(list_of), np.float32)
    z[np.argsort(list_of, kind="stable")] = np.concatenate([np.asarray(lists[i], np.float32) for i in idx])
    # the centre of the list (pixel centres are integers) and a jitter that keeps the 3 x 3-pixel rectangle inside the full part of it
    u = (list_of % lists_x) * LIST_W + 7.5 + rng.uniform(-3, 3, len(z))
    v = (list_of // lists_x) * LIST_H + 3.5 + rng.uniform(-1.5, 1.5, len(z))
    f = float(max(W, H, 64))
    z64 = z.astype(np.float64)
    pos = np.stack([(u - W / 2) / f * z64, (v - H / 2) / f * z64, z64], 1).astype(np.float32)
    pos[:, 2] = -z if behind else z
    n = len(z)
    s = list_scenes._pack(dict(pos=pos, scale_raw=np.full((n, 3), SCALE_RAW), q_raw=np.tile([1.0, 0, 0, 0], (n, 1)), opacity_raw=np.zeros(n),
                               f_dc=np.zeros((n, 3)), f_rest=np.zeros((n, 45))), H, W, f, f, W / 2.0, H / 2.0)
    s["list_of"] = list_of
    return s


# ---- the frames ------------------------------------------------------------------------------------------------------------
class Frame:
    """One frame: the scene, and per list (arrays over `lists`, ascending) its pattern, length, instantiation, intended path and
    intended shift (-1: not pinned)."""

    def __init__(self, name, H, W, spec, seed):
        """spec: [(pattern name, n, LOG2B for the range patterns or None = that of the list's own class)] -- dealt to random lists."""
        rng = np.random.default_rng(seed)
        n_lists = ((W + LIST_W - 1) // LIST_W) * ((H + LIST_H - 1) // LIST_H)
        assert len(spec) <= n_lists, (name, len(spec), n_lists)
        where = np.sort(rng.permutation(n_lists)[:len(spec)])
        self.name, self.H, self.W, self.n_lists = name, H, W, n_lists
        self.n_binned = sum(n for _, n, _ in spec)
        self.class0 = class0_rule(self.n_binned, n_lists)
        self.lists, self.pattern, self.length = where, [p for p, _, _ in spec], np.array([n for _, n, _ in spec])
        self.inst, self.path, self.shift, depths = [], [], [], {}
        for l_, (p, n, L) in zip(where, spec):
            inst, glob = instantiation(n, self.class0)
            T, E, own = INST[inst]
            bits, path, shift = pattern(p, rng, n, own if L is None else L)
            assert L is None or L == own, (name, p, n, "a range pattern is made for the LOG2B of its own class")
            self.inst.append(inst)
            self.path.append("C" if glob and n >= T * E else path)
            self.shift.append(-1 if shift is None or self.path[-1] == "C" else shift)
            depths[int(l_)] = bits.astype(np.uint32).view(np.float32)
        self.inst, self.path, self.shift = np.array(self.inst), np.array(self.path), np.array(self.shift)
        self.depths = depths
        self.seed = seed

    @functools.cached_property
    def scene(self):
        return build(self.H, self.W, self.depths, self.seed)

    def describe(self, k):
        return f"frame {self.name}, list {self.lists[k]} ({self.pattern[k]}, {self.length[k]} entries, sort_list<{self.inst[k]}> path {self.path[k]})"

    def summary(self):
        combos = sorted({f"{i}/{p}" for i, p in zip(self.inst, self.path)})
        return (f"{self.name}: {self.H} x {self.W} px, {self.n_lists} lists ({len(self.lists)} non-empty), {self.n_binned} pairs, class0 "
                f"{'launched' if self.class0 else 'not launched'}; paths {' '.join(combos)}")


def _every(lengths, patterns=ALL_PATTERNS, L=None):
    return [(p, n, L if p in RANGES else None) for n in lengths for p in patterns if applies(p, n)]


def _alternate(count, n):
    return [("spread" if k % 2 == 0 else "equal", n, None) for k in range(count)]


GLOBAL_PATTERNS = ("spread", "equal", "descending")
# name -> (H, W, spec).  REDUCED: the three frames of about 10^6 pairs at the size of the CPU placement check -- the same image, the
# same number of lists and the same alternation of patterns; only the lists are shorter.
_FRAMES = {
    "small": lambda: (64, 256, _every((1, 2, 3, 7, 8, 48, 49, 63, 64, 65, 128, 255), L=9)),
    "mid": lambda: (64, 256, _every((256, 257, 511, 512, 513, 1023), L=11)),
    # 102 390 pairs in 64 lists: class0 is true, the 512-thread kernel starts behind class 0's (empty) part of `order`
    "class1": lambda: (64, 128, _every((1024, 1025, 2047, 2048, 4095), L=12)),
    "class0": lambda: (64, 128, _every((4096, 4097, 8191), L=13) + _every((8192, 8193, 12289), GLOBAL_PATTERNS)),
    "no_class0": lambda: (256, 512, _every((4095, 4096, 5000), ("spread", "equal"))),
    "mixed": lambda: (72, 144, _every((100,), ("spread", "equal")) + _every((300,), ("spread", "equal")) + _every((2000,), ("spread", "equal"))
                      + _every((5000,), ("spread", "equal")) + _every((8200,), ("spread",))),
    "many_lists_4096": lambda: (128, 272, _alternate(257, 4096)),
    "many_lists_1024": lambda: (224, 448, _alternate(769, 1024)),
    "many_lists_256": lambda: (512, 1040, _alternate(4097, 256)),
    # every list of a 257 x 256-list image holds 1, 2 or 3 entries
    "many_lists_small": lambda: (2048, 4112, [(("spread", "equal")[k % 2], 1 + k % 3, None) for k in range(257 * 256)]),
}
REDUCED = {"many_lists_4096": lambda: (128, 272, _alternate(257, 64)), "many_lists_1024": lambda: (224, 448, _alternate(769, 64)),
           "many_lists_256": lambda: (512, 1040, _alternate(4097, 8))}
FRAMES = tuple(_FRAMES)
# the class whose launch must need a second grid-stride pass, and how many lists of it the frame holds at least
MANY = {"many_lists_4096": ("1024", 257), "many_lists_1024": ("512", 769), "many_lists_256": ("256", 4097), "many_lists_small": ("wave", 65537)}
EMPTY_IMAGES = ((512, 1024), (1024, 2064))       # 4096 lists (one round of the plan) and 16512 lists (two rounds)


@functools.lru_cache(maxsize=2)
def frame(name, reduced=False):
    H, W, spec = (REDUCED[name] if reduced else _FRAMES[name])()
    return Frame(name + (" (reduced)" if reduced else ""), H, W, spec, seed=1 + FRAMES.index(name))


def empty(hw):
    """Every Gaussian behind the camera: a few to each of 50 lists' directions."""
    H, W = hw
    rng = np.random.default_rng(9)
    n_lists = ((W + LIST_W - 1) // LIST_W) * ((H + LIST_H - 1) // LIST_H)
    lists = {int(l_): (BASE_BITS + np.arange(5)).astype(np.uint32).view(np.float32) for l_ in rng.permutation(n_lists)[:50]}
    return build(H, W, lists, seed=9, behind=True)
