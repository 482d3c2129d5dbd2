"""What every tools/bench_*.py shares: the paths, the data-sheet peaks, how a time is taken (host clock around a
synchronised call, device events around a window of calls, the library's launch record), the compile command of a kernel
file as the Makefile states it, the compiler's resource-usage record made with that command, and the JSON line.

A tool puts its own directory on sys.path and imports this module; what is left in the tool is its workload, its torch
comparison, its operation and byte counts and its record.  torch and dpc.render are imported inside the functions that
need them, so --resource-usage and a test that loads a tool without a device pay for neither."""
import json
import os
import re
import shlex
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-unsup-pc_amd")
CSRC = os.path.join(PKG, "csrc")
for _p in (ROOT, PKG, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# MI355X_MICROARCH.md: HBM bytes per second; vector (non-MFMA) operations per second, an fma counted as two
HBM_PEAK = 8.0e12
FP32_VECTOR_PEAK = 157.3e12
FP64_VECTOR_PEAK = 78.6e12


# --- wall time: a host clock around calls that end in a device synchronise ---------------------------------------------
def _synchronize():
    import torch

    torch.cuda.synchronize()


def walls_ms(fn, reps, warmup=1):
    """Milliseconds of each of `reps` calls of fn after `warmup` calls, each call ended by a device synchronise."""
    for _ in range(warmup):
        fn()
    _synchronize()
    times = []
    for _ in range(reps):
        _synchronize()
        t0 = time.perf_counter()
        fn()
        _synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


def stats(times, digits=3):
    """[median, min, max] of times, rounded to `digits` (None: as they are)."""
    out = [float(np.median(times)), float(min(times)), float(max(times))]
    return out if digits is None else [round(x, digits) for x in out]


def median_ms(fn, reps, warmup=1, digits=3):
    return stats(walls_ms(fn, reps, warmup), digits)


def upper_median(times):
    """The middle one of an odd number of times, the upper of the middle two of an even number."""
    return sorted(times)[len(times) // 2]


def alternate(fns, reps):
    """stats() of each fn of {name: fn} after one warm-up call of each, the variants taking turns within every round."""
    for fn in fns.values():
        fn()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            times[k] += walls_ms(fn, 1, warmup=0)
    return {k: stats(v) for k, v in times.items()}


def batch_host_ms(fn, reps, warmup=1):
    """(milliseconds per call of `reps` back-to-back calls ended by one synchronise, milliseconds per call the host spent
    issuing them), after `warmup` calls."""
    for _ in range(warmup):
        fn()
    _synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    host = time.perf_counter() - t0
    _synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, host * 1e3 / reps


def batch_ms(fn, reps, warmup=1):
    return batch_host_ms(fn, reps, warmup)[0]


# --- device events around a window of back-to-back calls ---------------------------------------------------------------
def event_ms(fn, reps):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def event_window_times(fns, reps, warmup, windows):
    """{name: [event_ms of each window]}: `warmup` calls of every fn of {name: fn} first (every shape the timed windows
    use), then `windows` rounds in which the fns take turns, a window of `reps` calls each."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    _synchronize()
    times = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            times[k].append(event_ms(fn, reps))
    return times


def event_windows(fns, reps, warmup, windows, digits=4):
    """({name: median window}, {name: [min, max]}) of event_window_times, rounded."""
    times = event_window_times(fns, reps, warmup, windows)
    return ({k: round(upper_median(v), digits) for k, v in times.items()},
            {k: [round(min(v), digits), round(max(v), digits)] for k, v in times.items()})


# --- the library's launch record ---------------------------------------------------------------------------------------
def kernel_ms(fn, dev, prefixes=()):
    """{kernel family: milliseconds, summed over its launches} of one call of fn, from the library's launch record; only
    the families that start with one of `prefixes`, when given."""
    from dpc.render import _native

    return {k: round(float(sum(v)), 4) for k, v in _native.profile_kernels(fn, dev).items()
            if not prefixes or k.startswith(prefixes)}


def share(amount, ms, peak, digits):
    """`amount` (bytes, operations) in `ms` milliseconds as a share of `peak` per second; None without a time."""
    return round(amount / (ms * 1e-3) / peak, digits) if ms else None


# --- the compile command and the compiler's resource usage -------------------------------------------------------------
def compile_command(source):
    """The argv the build runs for csrc/<source>, read from the Makefile by a dry run."""
    obj = os.path.splitext(source)[0] + ".o"
    out = subprocess.run(["make", "-C", CSRC, "-n", "-B", "--no-print-directory", obj], capture_output=True, text=True,
                         check=True).stdout
    for line in out.splitlines():
        argv = shlex.split(line)
        if "-c" in argv and argv[argv.index("-c") + 1:][:1] == [source]:
            return argv
    raise RuntimeError("the Makefile's dry run has no line that compiles %s:\n%s" % (source, out))


_REMARK = re.compile(r"remark: (?:\S+ )?\s*(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                     r"TotalSGPRs|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (.*?)(?: \[-Rpass|$)")


def usage_rows(remarks):
    """The compiler's -Rpass-analysis=kernel-resource-usage remarks as one line per kernel: VGPR / AGPR / SGPR / spills /
    scratch / occupancy / LDS."""
    kernels, cur = [], {}
    for line in remarks.splitlines():
        m = _REMARK.search(line)
        if not m:
            continue
        k, v = m.group(1), m.group(2).strip()
        if k == "Function Name":
            if cur:
                kernels.append(cur)
            cur = {"name": subprocess.run(["c++filt", v], capture_output=True, text=True).stdout.strip()}
        else:
            cur[k.replace(" Spill", "_spill").split(" ")[0].replace("Total", "")] = v
    if cur:
        kernels.append(cur)
    rows = []
    for r in kernels:
        n = re.sub(r"\(anonymous namespace\)::", "", r["name"])
        n = re.sub(r"\(.*", "", n).replace("void ", "")
        rows.append("%-34s vgpr=%-4s agpr=%-4s sgpr=%-4s sgpr_spill=%-4s vgpr_spill=%-4s scratch=%-5s occ=%-2s lds=%s"
                    % (n, r.get("VGPRs"), r.get("AGPRs"), r.get("SGPRs"), r.get("SGPRs_spill"), r.get("VGPRs_spill"),
                       r.get("ScratchSize"), r.get("Occupancy"), r.get("LDS")))
    return rows


def resource_usage(source, path, notes, keep=None):
    """Compile csrc/<source> with the build's own command plus the resource-usage remarks (the object goes to a temporary
    directory) and write to `path`, and print: the command, the tool's `notes` lines, and one row per kernel -- of the
    kernels whose name contains `keep`, when given."""
    argv = compile_command(source)
    o = argv.index("-o")
    argv = argv[:o] + argv[o + 2:]
    with tempfile.TemporaryDirectory() as tmp:
        res = subprocess.run(argv + ["-Rpass-analysis=kernel-resource-usage", "-o", os.path.join(tmp, "x.o")], cwd=CSRC,
                             capture_output=True, text=True, check=True)
    rows = [r for r in usage_rows(res.stderr) if keep is None or keep in r]
    text = "".join(l + "\n" for l in ["# csrc/%s, %s" % (source, " ".join(argv))] + list(notes) + rows)
    with open(path, "w") as fh:
        fh.write(text)
    print(text, end="")


# --- the record --------------------------------------------------------------------------------------------------------
def emit(record, path=None):
    """Print the record as one JSON line and append it to `path`, when given."""
    line = json.dumps(record)
    print(line, flush=True)
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")
