"""The per-chunk bookkeeping of the raster kernels (staging, queue cap, gather of the private slots, flush) at its edges, on frames
built BY HAND: records, ranges, launch order and sorted ids are written into project_state / bin_state by the test and handed to the
raster entries directly, so that every list holds exactly the entries its case needs.  A 64 x 48 image = 4 x 6 lists: a chunk
boundary cannot hide in a large frame.  Checked with tests/raster_oracle.py (composite, chunk_layout, check) at the bounds of
tests/test_gpu_raster.py: K = 3 x the ratio of the oracle's own float32 evaluation, per output kind; the absolute sums of the ABS
variants with tests/absgrad_oracle.py at the bound of tests/test_gpu_absgrad.py.

The hand-made frame (one frame, every case in lists of its own):
  lists of 0, 1, 63, 64, 65, 128 and 129 entries           chunk edges
  list MIXED: entries queued in all eight sub-tiles beside entries queued in one      the gather over an entry's sub-tiles
  list CAP: 40 of its first 64 entries in ONE sub-tile      the chunk is cut at the queue cap of the backward kernel
  list DIES: opaque layers over the whole list in front of 60 more entries: every pixel dies inside the first chunk, the loop stops
             short of the queues' ends, and the rows behind stay exact zeros
Beside it: n == 0 on a hand-made state, the all-empty scenes through the composite entries (whose launch order the plan kernel writes
by itself), and a frame rendered into a project_state that still holds a LARGER frame."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from tests import absgrad_oracle as ao
from tests import device_frame as dfm
from tests import list_scenes
from tests import raster_oracle as ro
from tests import util

pytestmark = pytest.mark.gpu
abi = dfm.abi
DEV = dfm.DEV
H, W = 48, 64
LX, LY = 4, 6
CHI, AMAX, CUT = (float(np.float32(x)) for x in (6.25, 0.99, 1 / 128.))
BG = (1.0, 0.5, 0.25)
K_LINEAR = 8.0                                   # tests/test_gpu_absgrad.py: the linear term's own roundings
EDGE_COUNTS = {0: 0, 1: 1, 2: 63, 3: 64, 4: 65, 5: 128, 6: 129}       # rows 0 and 1 of the 4 x 6 lists
MIXED, CAP, DIES = 7, 8, 21                      # row 1, row 2, and row 5: the opaque layers of DIES reach rows 3 to 5 only
N_LAYERS, N_BEHIND = 20, 60
_vp = dfm._vp


# ---- the frame ------------------------------------------------------------------------------------------------------------------------

def _record(u, v, sx, sy, o, rgb, z):
    """An axis-aligned Gaussian: conic diag(1 / sx^2, 1 / sy^2), box half-extents = the reach of {q <= chi} padded as the projection pads."""
    r = np.zeros(16, np.float64)
    r[0:6] = (u, v, 1.0 / sx ** 2, 0.0, 1.0 / sy ** 2, o)
    r[6:8] = (np.sqrt(CHI) * sx + 0.01, np.sqrt(CHI) * sy + 0.01)
    r[8:11], r[11] = rgb, z
    return r


def _origin(l_):
    return (l_ % LX) * ro.LIST_W, (l_ // LX) * ro.LIST_H


def hand_frame():
    """rec [n,16] float32 and, per list, the ids of its entries in depth order (every Gaussian is in the lists its box meets)."""
    rng = np.random.default_rng(17)
    recs = []

    def add(u, v, sx, sy, o):
        recs.append(_record(u, v, sx, sy, o, rng.uniform(0.05, 0.95, 3), rng.uniform(2.0, 9.0)))

    def small(l_, count, o=(0.03, 0.25)):                # inside ONE sub-tile of list l_, the sub-tiles taken in turn (64 of them: 8 per queue, far
        ox, oy = _origin(l_)                             # below the cap): sigma <= 0.4 -> reach <= 1.01 px around a centre <= 0.2 px off the sub-tile's
        for k in range(count):
            t = k % 8
            add(ox + 4 * (t & 3) + 1.5 + rng.uniform(-0.2, 0.2), oy + 4 * (t >> 2) + 1.5 + rng.uniform(-0.2, 0.2), rng.uniform(0.3, 0.4), rng.uniform(0.3, 0.4),
                rng.uniform(*o))

    for l_, c in EDGE_COUNTS.items():
        small(l_, c)
    ox, oy = _origin(MIXED)                              # 100 entries: every third one reaches all 8 sub-tiles, the others sit in one
    for k in range(100):
        if k % 3 == 0:
            add(ox + 7.5 + rng.uniform(-0.3, 0.3), oy + 3.5 + rng.uniform(-0.2, 0.2), 2.2, 0.9, rng.uniform(0.03, 0.12))
        else:
            t = int(rng.integers(8))
            add(ox + 4 * (t & 3) + 1.5, oy + 4 * (t >> 2) + 1.5, 0.5, 0.5, rng.uniform(0.05, 0.3))
    ox, oy = _origin(CAP)                                # 80 entries; 40 of the first 64 (by depth: below) inside sub-tile (1, 0)
    n_cap0 = len(recs)
    for k in range(80):
        if k < 64 and k % 8 < 5:
            add(ox + 5.5 + rng.uniform(-0.2, 0.2), oy + 1.5 + rng.uniform(-0.2, 0.2), 0.5, 0.5, rng.uniform(0.02, 0.08))
        else:
            small(CAP, 1)
    for k in range(80):
        recs[n_cap0 + k][11] = 2.0 + 0.05 * k           # depth order = order of creation
    ox, oy = _origin(DIES)                               # 20 opaque layers (alpha >= 0.53 on every pixel of the list: T < 5e-5 behind 16 of
    for k in range(N_LAYERS):                            # them; they reach rows 3 to 5 of the lists), then 60 small ones behind
        add(ox + 7.5 + rng.uniform(-0.3, 0.3), oy + 3.5 + rng.uniform(-0.3, 0.3), 12.0, 6.0, 0.97)
        recs[-1][11] = 1.0 + 0.01 * k
    n0 = len(recs)
    small(DIES, N_BEHIND)
    for k in range(n0, len(recs)):
        recs[k][11] += 10.0
    small(11, 5)
    small(20, 30)
    rec = np.asarray(recs, np.float32)
    lists = [[] for _ in range(LX * LY)]
    for i, r in enumerate(rec.astype(np.float64)):
        for l_ in range(LX * LY):
            ox, oy = _origin(l_)
            if r[0] + r[6] >= ox and r[0] - r[6] <= ox + ro.LIST_W - 1 and r[1] + r[7] >= oy and r[1] - r[7] <= oy + ro.LIST_H - 1:
                lists[l_].append(i)
    lists = [sorted(m, key=lambda i: (rec[i, 11], i)) for m in lists]
    return rec, lists


class HandFrame(dfm.Frame):
    """tests/device_frame.Frame on a state written by the test: rec, ranges, order (longest list first), the Gaussians' rectangles,
    masks and list counts (the deterministic backward numbers a Gaussian's rows by them) and the sorted ids; forward() / backward() and
    the canaries are Frame's."""

    def __init__(self, rec, lists, H=H, W=W):
        self.lib = abi.lib()
        self.s = dict(H=H, W=W)
        self.n = n = len(rec)
        self.view = abi.make_view(H, W, 50.0, 50.0, W / 2, H / 2)
        self.lay = lay = abi.StateLayout()
        abi.check(self.lib.gsplat_project_state_layout(max(n, 1), C.byref(self.view), C.byref(lay)), "gsplat_project_state_layout")
        nl, lx = int(lay.lists), int(lay.lists_x)
        assert nl == len(lists)
        self.st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        raw = np.zeros(lay.bytes, np.uint8)

        def put(off, a):
            b = np.ascontiguousarray(a).view(np.uint8).ravel()
            raw[off:off + len(b)] = b
        lens = np.array([len(m) for m in lists], np.int64)
        ends = np.cumsum(lens)
        self.ranges = np.stack([ends - lens, ends], 1).astype(np.uint32)
        self.sorted_ids = np.array([i for m in lists for i in m], np.uint32)
        self.capacity = max(int(ends[-1]), 1)
        rect, mask, tiles = np.zeros((max(n, 1), 2), np.uint32), np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        member = [[] for _ in range(n)]
        for l_, m in enumerate(lists):
            for i in m:
                member[i].append(l_)
        for i, ls in enumerate(member):
            if not ls:
                continue
            xs, ys = [l_ % lx for l_ in ls], [l_ // lx for l_ in ls]
            x0, x1, y0, y1 = min(xs), max(xs), min(ys), max(ys)
            assert (x1 - x0 + 1) * (y1 - y0 + 1) <= 32
            rect[i] = (x0 | (y0 << 16), x1 | (y1 << 16))
            tiles[i] = len(ls)
            for x, y in zip(xs, ys):
                mask[i] |= np.uint32(1) << np.uint32((y - y0) * (x1 - x0 + 1) + (x - x0))
        if n:
            put(lay.rec, np.asarray(rec, np.float32))
        put(lay.rect, rect), put(lay.tiles, tiles), put(lay.mask, mask), put(lay.ranges, self.ranges)
        put(lay.order, np.argsort(-lens, kind="stable").astype(np.uint32))
        self.state = torch.tensor(raw, device=DEV)
        self.blay = abi.BinLayout()
        abi.check(self.lib.gsplat_bin_state_layout(self.capacity, C.byref(self.view), C.byref(self.blay)), "gsplat_bin_state_layout")
        b = np.zeros(self.blay.bytes + dfm.CANARY, np.uint8)
        b[self.blay.bytes:] = dfm.CANARY_BYTE
        ids = np.zeros(self.capacity, np.uint32)
        ids[:len(self.sorted_ids)] = self.sorted_ids
        b[self.blay.sorted_ids:self.blay.sorted_ids + 4 * self.capacity] = ids.view(np.uint8)
        self.bin_state = torch.tensor(b, device=DEV)
        self.scratch_bytes = 0
        self.scratch = torch.full((dfm.CANARY,), dfm.CANARY_BYTE, dtype=torch.uint8, device=DEV)
        self.sorted_ids = ids

    def pair_mask(self):
        return self.bin_state[self.blay.pair_mask:self.blay.pair_mask + self.capacity].cpu().numpy()

    def backward_abs(self, g_img, g_depth=None, g_alpha=None, aux=False, det=False, bg=None):
        """gsplat_rasterize_backward[_aux]_abs on a grad2d full of 0xFF bytes; returns grad2d [n,16]."""
        dev = {k: torch.tensor(np.ascontiguousarray(a, np.float32), device=DEV) for k, a in (("gi", g_img), ("gd", g_depth), ("ga", g_alpha)) if a is not None}
        g2d = self._buf("grad2d", self.n * 64)
        nbytes = (self.lib.gsplat_rasterize_backward_aux_abs_scratch_bytes if aux else self.lib.gsplat_rasterize_backward_abs_scratch_bytes)(self.n, self.capacity)
        scratch = self._buf("det_scratch", nbytes) if det else None
        acc = _vp(self.bufs["accum"][0])
        if not aux:
            abi.check(self.lib.gsplat_rasterize_backward_abs(self.n, self.capacity, C.byref(self.view), _vp(self.state), _vp(self.bin_state), acc, _vp(dev["gi"]), g2d,
                                                             0, scratch, nbytes if det else 0, self.st), "gsplat_rasterize_backward_abs")
        else:
            bgp = None if bg is None else (C.c_float * 3)(*bg)
            abi.check(self.lib.gsplat_rasterize_backward_aux_abs(self.n, self.capacity, C.byref(self.view), _vp(self.state), _vp(self.bin_state), acc,
                                                                 _vp(self.bufs["accum_aux"][0]), _vp(dev["gi"]), _vp(dev["gd"]), _vp(dev["ga"]), bgp, g2d, 0,
                                                                 scratch, nbytes if det else 0, self.st), "gsplat_rasterize_backward_aux_abs")
        torch.cuda.synchronize()
        return self._floats("grad2d", (self.n, 16))


def _upstream():
    rng = np.random.default_rng(3)
    return [rng.normal(0, 1, shape).astype(np.float32) for shape in ((H, W, 3), (H, W), (H, W))]


class _Run:
    """The hand-made frame once: forward plain / aux, the backward in its eight variants, the references with their K."""

    def __init__(self):
        self.rec, self.lists = hand_frame()
        fr = self.fr = HandFrame(self.rec, self.lists)
        up = self.up = _upstream()
        self.fwd, self.box, self.g2d, self.g2d_abs, self.intact = {}, {}, {}, {}, []
        for aux in (False, True):
            kw = dict(aux=aux, bg=BG if aux else None)
            self.box[aux] = fr.forward(accum=False, **kw)
            self.fwd[aux] = fr.forward(accum=True, **kw)
            self.intact.append(fr.canaries_intact())
            for det in (False, True):
                mode = ("aux " if aux else "") + ("deterministic" if det else "atomic")
                bk = dict(g_img=up[0], g_depth=up[1] if aux else None, g_alpha=up[2] if aux else None, det=det, **kw)
                self.g2d[mode] = fr.backward(**bk)
                self.intact.append(fr.canaries_intact())
                self.g2d_abs[mode] = fr.backward_abs(**bk)
                self.intact.append(fr.canaries_intact())
        self.pair_mask = fr.pair_mask()
        self.args = (self.rec, fr.ranges, fr.sorted_ids, LX, H, W, CHI, AMAX, CUT)
        self.ref, self.K, self.ab = {}, {}, {}
        for aux in (False, True):
            kw = dict(g_img=up[0], g_depth=up[1], g_alpha=up[2], bg=BG, aux=True) if aux else dict(g_img=up[0])
            self.ref[aux] = ro.composite(*self.args, **kw)
            cal = ro.ratios(ro.composite_f32(*self.args, **kw), self.ref[aux])
            self.K[aux] = {k: 3.0 * cal.get(k, 0.0) for k in ro.KINDS}
            kw.pop("aux", None)
            self.ab[aux] = ao.absgrad(self.ref[aux], self.rec, chi=CHI, alpha_max=AMAX, alpha_cutoff=CUT, **kw)


_RUN = []


def _run():
    """(A failed set-up is kept and raised again: nothing runs on the device a second time.)"""
    if not _RUN:
        try:
            _RUN.append(_Run())
        except Exception as e:
            _RUN.append(e)
    if isinstance(_RUN[0], Exception):
        raise _RUN[0]
    return _RUN[0]


MODES = ("atomic", "deterministic", "aux atomic", "aux deterministic")


# ---- the frame holds the cases it was made for ---------------------------------------------------------------------------------------

def test_the_frame_holds_its_cases():
    run = _run()
    lens = run.fr.ranges[:, 1].astype(np.int64) - run.fr.ranges[:, 0]
    for l_, c in EDGE_COUNTS.items():
        assert lens[l_] == c, f"list {l_}: {lens[l_]} entries, made for {c}"
    pm, rg = run.pair_mask, run.fr.ranges
    bits = np.array([bin(int(m)).count("1") for m in pm])
    mixed = bits[rg[MIXED, 0]:rg[MIXED, 1]]
    assert lens[MIXED] == 100 and (mixed == 8).sum() >= 30 and (mixed == 1).sum() >= 60, "entries in all eight sub-tiles beside entries in one"
    first = pm[rg[CAP, 0]:rg[CAP, 0] + 64]
    assert max(int(((first >> t) & 1).sum()) for t in range(8)) >= 25, "one sub-tile holds 25 or more of 64 consecutive entries"
    _, _, chunks = ro.chunk_layout(rg, pm)
    cut = [c for c in chunks if c[3]]
    assert any(c[0] == CAP for c in cut), "the chunk of list CAP is cut at the queue cap"
    assert any(c[0] == DIES for c in cut), "the opaque layers of list DIES fill all eight queues"
    assert not any(c[3] for c in chunks if c[0] in EDGE_COUNTS), "the lists of the chunk edges are cut at 64 entries and nowhere else"
    assert {c[2] for c in chunks if c[0] in EDGE_COUNTS} >= {1, 63, 64}, "whole chunks, a chunk of 63 and chunks of one entry"
    # list DIES: every pixel is dead before the 24 entries of its first chunk are through, and the 60 entries behind get nothing
    alive = run.ref[False].dec["alive"]
    s0 = int(rg[DIES, 0])
    assert not alive[s0 + 16:int(rg[DIES, 1])].any() and alive[s0].all()
    behind = run.fr.sorted_ids[s0 + N_LAYERS:int(rg[DIES, 1])]
    assert len(behind) == N_BEHIND and not run.ref[False].scale[behind].any()


# ---- forward ---------------------------------------------------------------------------------------------------------------------------

def test_forward():
    run = _run()
    for aux in (False, True):
        out = run.fwd[aux]
        r = ro.check(out, run.ref[aux], run.K[aux], f"hand-made frame, forward{' aux' if aux else ''}")
        print(f"forward{' aux' if aux else ''}: device |delta| / (2^-24 scale) {r}; K {run.K[aux]}")
        for k in run.box[aux]:                          # box-test queues (no backward to follow) against the exact test's: the same bits
            assert np.array_equal(run.box[aux][k].view(np.uint32), out[k].view(np.uint32)), f"{k}: box-test forward differs"


# ---- backward: plain, deterministic, AUX -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_backward(mode):
    run = _run()
    aux = mode.startswith("aux")
    ref, K = run.ref[aux], run.K[aux]
    r = ro.check(dict(grad2d=run.g2d[mode]), ref, K, f"hand-made frame, backward {mode}", pair_mask=run.pair_mask)
    print(f"backward {mode}: device |delta| / (2^-24 scale) {r}; K {K}")
    behind = run.fr.sorted_ids[int(run.fr.ranges[DIES, 0]) + N_LAYERS:int(run.fr.ranges[DIES, 1])]
    assert not run.g2d[mode][behind].any(), "rows behind the entry at which list DIES ended must stay exact zeros"
    if "deterministic" not in mode:
        other = run.g2d[mode.replace("atomic", "deterministic")]
        kk = np.array([K["moments"]] * 6 + [K["colour"]] * (ref.ns - 6))
        d = np.abs(run.g2d[mode].astype(np.float64) - other)[:, :ref.ns]
        bad = np.argwhere(d > kk[None, :] * ro.EPS * ref.scale + ref.allow)
        assert not len(bad), f"{mode} against deterministic: Gaussian {bad[0][0]}, column {bad[0][1]}: |delta| {d[tuple(bad[0])]:.3e}"


def test_single_list_rows_agree_bit_for_bit_between_the_two_flushes():
    """A Gaussian that lies in ONE list has one row: the atomic flush adds it to a zero, the deterministic flush stores it and
    pair_reduce_kernel adds it to a zero.  The two must agree in every bit, whether the row was gathered from one sub-tile or from eight."""
    run = _run()
    single = np.array([sum(i in m for m in run.lists) == 1 for i in range(run.fr.n)])
    assert single.sum() > 500
    for aux in (False, True):
        a, d = run.g2d[("aux " if aux else "") + "atomic"], run.g2d[("aux " if aux else "") + "deterministic"]
        diff = np.argwhere(a[single].view(np.uint32) != d[single].view(np.uint32))
        assert not len(diff), f"aux {aux}: {len(diff)} values of single-list rows differ between the atomic and the deterministic run"


# ---- backward: ABS ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_backward_abs(mode):
    run = _run()
    aux = mode.startswith("aux")
    ns = 10 if aux else 9
    g, plain, ref, K = run.g2d_abs[mode], run.g2d[mode], run.ref[aux], run.K[aux]
    assert np.isfinite(g).all()
    assert not g[:, 12:].any() and (aux or not g[:, 9].any()), "columns 12-15 (and 9 without aux) are exact zeros"
    if "deterministic" in mode:
        diff = np.argwhere(g[:, :ns].view(np.uint32) != plain[:, :ns].view(np.uint32))
        assert not len(diff), f"{mode}: {len(diff)} values of columns 0-{ns - 1} differ from the plain entry, first at {diff[0]}"
    else:
        low = g.copy()
        low[:, 10:12] = 0.0
        ro.check(dict(grad2d=low), ref, K, f"hand-made frame, _abs backward {mode}", pair_mask=run.pair_mask)
    ab = run.ab[aux]
    assert (g[:, 10:12] >= 0).all() and (ab.S > 0).any()
    assert not g[~ab.in_list].any()
    d = np.abs(g[:, 10:12].astype(np.float64) - ab.S)
    bad = np.argwhere(d > (K["moments"] + K_LINEAR) * ro.EPS * ab.scale + ab.allow)
    assert not len(bad), (f"{mode}: Gaussian {bad[0][0]}, column {10 + bad[0][1]}: {g[bad[0][0], 10 + bad[0][1]]!r}, oracle {ab.S[tuple(bad[0])]!r}, "
                          f"|delta| {d[tuple(bad[0])]:.3e}, scale {ab.scale[tuple(bad[0])]:.3e}; {len(bad)} beyond the bound")


def test_canaries():
    run = _run()
    assert len(run.intact) == 2 * (1 + 2 * 2) and all(run.intact)


# ---- n == 0, all-empty scenes ------------------------------------------------------------------------------------------------------------

def test_no_gaussians_on_a_hand_made_state():
    """n == 0: every list empty, the launch order still a permutation of the lists.  The forward writes every pixel (zeros, or the
    clamped background), the backward entries return without touching anything."""
    fr = HandFrame(np.zeros((0, 16), np.float32), [[] for _ in range(LX * LY)])
    out = fr.forward(accum=True)
    assert not out["image"].any() and not out["accum"].any()
    out = fr.forward(accum=True, aux=True, bg=(2.0, 0.5, -1.0))
    assert np.array_equal(out["image"], np.broadcast_to(np.float32([1.0, 0.5, 0.0]), (H, W, 3)))
    assert not out["depth"].any() and not out["alpha"].any() and not out["accum"].any() and not out["accum_aux"].any()
    up = _upstream()
    for det in (False, True):
        fr.fwd_aux = False
        fr.backward(up[0], det=det)
        fr.backward_abs(up[0], det=det)
    assert fr.canaries_intact()


@pytest.mark.parametrize("name", util.EMPTY_CASES)
def test_all_empty_scene_through_the_composite_entries(gs, name):
    """Nothing is binned: the plan kernel runs by itself and must leave what the raster kernels start from."""
    d = util.load(name)
    for det in (False, True):
        old = gs.ops.set_deterministic(det)
        try:
            p = util.tensors(d, torch.float32, device=DEV, grad=True)
            with gs.deferred_checks() as chk:
                img = gs.render_gaussians(*[p[k] for k in list_scenes.NAMES], torch.tensor(d["c2w"], device=DEV), *util.cam_args(d), **d["kwargs"])
                img.sum().backward()
            chk.verify()
            torch.cuda.synchronize()
        finally:
            gs.ops.set_deterministic(old)
        assert img.shape == (d["H"], d["W"], 3) and float(img.detach().abs().max()) == 0.0
        assert all(t.grad is not None and float(t.grad.abs().max()) == 0.0 for t in p.values())


# ---- a smaller frame into a state that held a larger one ----------------------------------------------------------------------------------

def _scene(hw, f):
    """400 Gaussians over the image; the same ones for every (hw, f) with the same W / f and H / f."""
    rng = np.random.default_rng(41)
    n = 400
    z = rng.uniform(3, 6, n)
    uv = rng.uniform(0, 1, (n, 2)) - 0.5
    pos = np.stack([uv[:, 0] * hw[1] / f * z, uv[:, 1] * hw[0] / f * z, z], 1)
    d = dict(pos=pos, scale_raw=np.log(rng.uniform(0.05, 0.25, (n, 3))), q_raw=rng.normal(0, 1, (n, 4)), opacity_raw=rng.uniform(-2.0, 1.0, n),
             f_dc=0.5 * rng.normal(0, 1, (n, 3)), f_rest=0.1 * rng.normal(0, 1, (n, 45)))
    return list_scenes._pack(d, hw[0], hw[1], f, f, hw[1] / 2.0, hw[0] / 2.0)


def _frame_outputs(fr, state):
    """project (into `state`, as it is), bin, forward, deterministic backward of fr's scene."""
    fr.state = state
    host = torch.full((C.sizeof(abi.Counts),), 255, dtype=torch.uint8).pin_memory()
    abi.check(fr.lib.gsplat_project(C.byref(fr.g), _vp(fr.c2w), C.byref(fr.view), _vp(fr.state), _vp(fr.block), fr.block.numel(),
                                    C.c_void_p(host.data_ptr()), None, dfm.F, fr.st), "gsplat_project")
    torch.cuda.synchronize()
    counts = abi.Counts.from_buffer_copy(host.numpy().tobytes())
    assert counts.n_binned > 0
    fr.binned = False
    fr.bin(counts.n_binned)
    out = fr.forward(accum=True)
    g = fr.backward(list_scenes.upstream(fr.s)[0], det=True)
    return counts.n_binned, out, g


def test_a_smaller_frame_into_the_state_of_a_larger_one():
    """256 x 192 (384 lists), then 64 x 48 (24 lists) of the same Gaussians into the same project_state: the arrays move (their offsets
    depend on the number of lists), so whatever the small frame does not write itself is the large frame's data at another meaning.
    The result must be the one of a cleared state, bit for bit."""
    big, small = dfm.Frame(_scene((192, 256), 200.0)), dfm.Frame(_scene((48, 64), 50.0))
    assert small.lay.bytes < big.lay.bytes and small.lay.order != big.lay.order
    state = torch.zeros(big.lay.bytes, dtype=torch.uint8, device=DEV)
    nb_big, _, _ = _frame_outputs(big, state)
    nb_dirty, out_dirty, g_dirty = _frame_outputs(small, state)
    fresh = dfm.Frame(_scene((48, 64), 50.0))
    nb_fresh, out_fresh, g_fresh = _frame_outputs(fresh, torch.zeros(big.lay.bytes, dtype=torch.uint8, device=DEV))
    assert nb_big > 0 and nb_dirty == nb_fresh
    for k in out_fresh:
        assert np.array_equal(out_dirty[k].view(np.uint32), out_fresh[k].view(np.uint32)), f"{k} differs from the cleared state's"
    assert np.array_equal(g_dirty.view(np.uint32), g_fresh.view(np.uint32)), "grad2d differs from the cleared state's"
    assert out_fresh["image"].any() and g_fresh.any()
    assert small.canaries_intact() and fresh.canaries_intact()
