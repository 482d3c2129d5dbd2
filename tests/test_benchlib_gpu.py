"""tools/benchlib.py on the device: each timing helper runs its function as often as it says and returns times that make
sense (positive, finite, median within the spread), and kernel_ms reads the library's launch record."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import benchlib as BL  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture
def counted():
    """(fn, calls): fn adds 1 in place to a 1,024-element device tensor, calls() is how often it ran."""
    x = torch.zeros(1024, device="cuda")

    def fn():
        x.add_(1)

    return fn, lambda: int(x[0].item())


def test_walls_ms_runs_warmup_plus_reps(counted):
    fn, calls = counted
    times = BL.walls_ms(fn, 3, warmup=1)
    assert len(times) == 3 and all(math.isfinite(t) and t > 0 for t in times)
    assert calls() == 4


def test_alternate_times_every_variant(counted):
    fn, calls = counted
    out = BL.alternate({"a": fn, "b": fn}, 2)
    assert sorted(out) == ["a", "b"]
    for med, lo, hi in out.values():
        assert 0 < lo <= med <= hi and math.isfinite(hi)
    assert calls() == 2 + 2 * 2                       # one warm-up call of each, then two rounds of both


def test_event_windows_median_lies_in_its_spread(counted):
    fn, calls = counted
    med, spread = BL.event_windows({"a": fn}, reps=4, warmup=1, windows=3)
    assert sorted(med) == sorted(spread) == ["a"]
    lo, hi = spread["a"]
    assert 0 < lo <= med["a"] <= hi and math.isfinite(hi)
    assert calls() == 1 + 3 * 4


def test_kernel_ms_reads_the_launch_record():
    import dpc.render as R

    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(1)
    vs, vt = (torch.rand(64, 3, generator=g) - 0.5).to(dev), (torch.rand(64, 3, generator=g) - 0.5).to(dev)
    every = BL.kernel_ms(lambda: R.point_cloud_distance(vs, vt), dev)
    nearest = BL.kernel_ms(lambda: R.point_cloud_distance(vs, vt), dev, "k_nearest")
    assert nearest and all(k.startswith("k_nearest") and ms > 0 for k, ms in nearest.items())
    assert set(nearest) <= set(every) and BL.kernel_ms(lambda: R.point_cloud_distance(vs, vt), dev, "k_no_such") == {}
