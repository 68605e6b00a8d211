"""bench.py's plain run and --dump-outputs: the line carries the headline figures only, --steps sets the timed steps, and the
dumped arrays are what the timed path returned in its last step (the same frame rendered here)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}


def test_zero_steps_is_refused():
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--steps" in r.stderr
    assert not any(l.startswith("{") for l in r.stdout.splitlines())


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(gs, tmp_path):
    import torch
    import bench
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--config", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                       env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "Mpix/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32"
    assert not {"roofline", "stages", "cpu_baseline", "sustained", "host_queue_ms"} & set(d), "extras belong to --full"
    files = sorted(os.listdir(out))
    assert files == sorted(["image.npy"] + ["grad_" + k + ".npy" for k in bench.NAMES]), files   # config 1 is small: nothing sampled
    got = {f[:-4]: np.load(out / f) for f in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())

    params, cam = bench.synthetic_scene(1)
    dev = torch.device("cuda:0")
    p = {k: params[k].to(dev).requires_grad_(True) for k in bench.NAMES}
    gimg = torch.rand(cam["H"], cam["W"], 3, generator=torch.Generator().manual_seed(1)).to(dev)
    img = gs.render_gaussians(*[p[k] for k in bench.NAMES], bench.orbit_c2w(0).to(dev), cam["H"], cam["W"], cam["fx"], cam["fy"],
                              cam["cx"], cam["cy"])
    img.backward(gimg)
    torch.cuda.synchronize()
    assert np.abs(got["image"] - img.detach().cpu().numpy()).max() <= 1e-6
    for k in bench.NAMES:                          # (gradients: equal up to the order of the float atomics)
        ref = p[k].grad.cpu().numpy()
        assert got["grad_" + k].shape == ref.shape, k
        assert np.linalg.norm(got["grad_" + k] - ref) <= 1e-5 * np.linalg.norm(ref) + 1e-30, k
