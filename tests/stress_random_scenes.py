#!/usr/bin/env python3
"""One-off stress (a tool, not a test; needs a GPU): tests/test_gpu_parity.py::test_random_scenes_vs_oracle over many more seeds, or
-- with --modes -- the sweep of tests/test_gpu_mode_scenes.py (every row of tests/mode_scenes.MODES) over them.
    python tests/stress_random_scenes.py [--modes] [first_seed] [count]          (--modes without seeds: the test's own seeds)
A failure whose message is a tolerance overshoot by a few percent is usually the reference's own fp32 arithmetic
(tests/debug_seed.py <seed> [row] shows the oracle-in-float32 errors beside the HIP ones); anything else is a bug.
--modes also prints, over all cases, the worst image, depth, alpha and gradient errors of the HIP path beside the float32 oracle's.
Only a failed assertion is counted and passed over: any other exception (a device error among them) ends the run."""
import contextlib
import importlib
import io
import sys

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from tests import mode_scenes as ms

gs = importlib.import_module("3d-gaussian-splatting-for-novel-view-synthesis_amd")
args = [a for a in sys.argv[1:] if a != "--modes"]
modes = "--modes" in sys.argv[1:]
first = int(args[0]) if len(args) > 0 else (0 if modes else 100)
count = int(args[1]) if len(args) > 1 else 80
worst = {}


def mode_case(seed, row):
    """One case with the test's checks (no entry of KNOWN_CORNERS applies beyond the test's seeds); folds its errors into `worst`."""
    import tests.test_gpu_mode_scenes as T
    m, d = ms.MODES[row], ms.mode_scene(seed)
    try:
        ref, cal = ms.oracle(d, m, ms.F64), ms.oracle(d, m, ms.F32)
    except Exception as e:
        assert str(e) == ms.tp.OFFSCREEN_MSG
        return T.test_random_scene_in_a_mode_vs_oracle(gs, seed, row)         # (the device must raise the same)
    got = ms.render_hip(gs, d, m)
    for tag, res in (("hip", got), ("float32 oracle", cal)):
        for what, e in ms.case_errors(res, ref, m).items():
            worst[what, tag] = max(worst.get((what, tag), (0.0,)), e + (f"seed {seed} row {row}",))
    known = T.KNOWN_CORNERS.get((seed, row))
    band = ms.threshold_band(d, m, known["band"], (known["threshold"],)) if known else None
    with contextlib.redirect_stdout(io.StringIO()):
        ms.check_case(got, ref, cal, m, f"seed {seed} row {row}", band=band)


bad = total = 0
for seed in (ms.SEEDS if modes and not args else range(first, first + count)):
    for row in (range(len(ms.MODES)) if modes else (None,)):
        total += 1
        try:
            if modes:
                mode_case(seed, row)
            else:
                import tests.test_gpu_parity as T
                T.test_random_scenes_vs_oracle(gs, seed)
        except AssertionError as e:
            bad += 1
            print("seed", seed, "" if row is None else f"row {row}", "FAILED:", str(e)[:300], flush=True)
    if (seed - first) % 50 == 49:
        print("...", seed - first + 1, "done", flush=True)
for what in sorted({k[0] for k in worst}):
    print("worst %-20s hip %s | float32 oracle %s" % (what, worst[what, "hip"], worst[what, "float32 oracle"]))
print("done, failures:", bad, "of", total)
