"""DspMat.interpolatef over all rows in one launch (interp.hip's k_mat_interpf_* kernels), with a shared delay and with one
delay per row, against the parent commit's one-launch-per-row route, the get_row -> DspVec.interpolatef -> set_row loop
and one vector call over the same number of points; and the vector call itself against the parent commit's, which must
not pay for the row dimension -> profiles/mat_interpf.txt.

  tools/build_baseline.sh HEAD~1        # the parent commit's library -> tools/lab/old_lib/libbasic_dsp_hip_B.so
  python tools/mat_interpf_bench.py --out profiles/mat_interpf.txt

Timing (the protocol of tools/mat_interp_bench.py): every case is warmed; a figure is the mean over windows that add up
to at least 0.3 s, each window one call on a fresh matrix (the row length changes; copied on the device, untimed) and
one device synchronisation, so the figure includes growing the matrix's buffers, as a user's first call does.  The two
libraries alternate in processes of their own (BDSP_HIP_LIBRARY), two rounds each; the smaller mean is shown.  The row
loop is timed on LOOP_ROWS rows and reported per row.  The vector tools (tools/interp_bench.py, tools/c4b_bench.py,
tools/interp_frac_bench.py) run the same way, parent - tree - parent - tree; the spread between the two runs of the
parent library is the allowance for the tree's mean.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BASELINE = os.path.join(ROOT, "tools", "lab", "old_lib", "libbasic_dsp_hip_B.so")
LOOP_ROWS = 256
WINDOW = 0.3
SHAPES = ((16384, 1000), (256, 65536))  # rows x complex f32 points
SINC, RC = 0, 1
# (label, function, roll-off, factor, conv_len)
CASES = (("x4 blocked", SINC, 0.0, 4.0, 12), ("x5 table", SINC, 0.0, 5.0, 12), ("x48/44.1 rc frac", RC, 0.35, 48.0 / 44.1, 12))
VECTOR_TOOLS = ("tools/interp_bench.py", "tools/c4b_bench.py", "tools/interp_frac_bench.py")


def worker():
    import numpy as np
    import basic_dsp_amd as bd
    bd.require_gpu()
    sync = lambda: bd.lib.bdsp_hip_synchronize(None)  # noqa: E731
    has_delays = hasattr(bd.lib, "bdsp_hip_mat_interpolatef_delays32")

    def single_time(make, fn, min_time=WINDOW):
        fn(make())
        sync()
        total, count = 0.0, 0
        while total < min_time:
            obj = make()
            sync()
            t0 = time.perf_counter()
            fn(obj)
            sync()
            total += time.perf_counter() - t0
            count += 1
        return total / count

    res = {}
    for rows, points in SHAPES:
        rng = np.random.default_rng(rows + points)
        tile = rng.uniform(-1.0, 1.0, (min(rows, 512), 2 * points))
        x = np.ascontiguousarray(np.resize(tile, (rows, 2 * points))).astype(np.float32)
        master, smaster = bd.DspMat(x, is_complex=True), bd.DspMat(x[:LOOP_ROWS], is_complex=True)
        vmaster = bd.DspVec(x.ravel(), is_complex=True)
        del x
        delays = np.linspace(-0.5, 0.5, rows).astype(np.float32)

        def fresh(src, r):
            f = bd.DspMat(rows=r, row_len=2 * points, is_complex=True, dtype=np.float32)
            f.add(src)
            return f

        def fresh_vec():
            return vmaster.clone()
        for label, fid, ro, factor, L in CASES:
            key = "%d x %d %s" % (rows, points, label)

            def shared(m):
                assert m.interpolatef(fid, factor, 0.25, L, ro) == 0

            def per_row(m):
                assert m.interpolatef(fid, factor, delays, L, ro) == 0

            def loop(ms):
                probe = ms.get_row(0)
                assert probe.interpolatef(fid, factor, 0.25, L, ro) == 0
                dst = bd.DspMat(rows=LOOP_ROWS, row_len=len(probe), is_complex=True, dtype=np.float32)
                for r in range(LOOP_ROWS):
                    v = ms.get_row(r)
                    assert v.interpolatef(fid, factor, 0.25, L, ro) == 0
                    assert dst.set_row(r, v) == 0
            res[key + " | shared"] = single_time(lambda: fresh(master, rows), shared) * 1e6
            if has_delays:
                res[key + " | per-row"] = single_time(lambda: fresh(master, rows), per_row) * 1e6
            res[key + " | vector"] = single_time(fresh_vec, lambda v: v.interpolatef(fid, factor, 0.25, L, ro)) * 1e6
            res[key + " | loop/row"] = single_time(lambda: fresh(smaster, LOOP_ROWS), loop) / LOOP_ROWS * 1e6
        del master, smaster, vmaster
    print("RESULT " + json.dumps(res), flush=True)


def run_with(lib, args):
    env = dict(os.environ)
    if lib:
        env["BDSP_HIP_LIBRARY"] = lib
    else:
        env.pop("BDSP_HIP_LIBRARY", None)
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit("%s failed (%d):\n%s" % (" ".join(args), r.returncode, (r.stdout + r.stderr)[-3000:]))
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--skip-vector", action="store_true", help="leave out the A/B of the vector tools")
    a = ap.parse_args()
    if a.worker:
        return worker()
    if not os.path.exists(BASELINE):
        raise SystemExit("no baseline library: run tools/build_baseline.sh <parent commit> first")
    out = []
    w = lambda s: (print(s, flush=True), out.append(s))  # noqa: E731
    w("# interpolatef of the rows of a matrix in one launch (k_mat_interpf_*, interp.hip) on one MI355X: tools/mat_interpf_bench.py.")
    w("# complex f32 rows; one call on a fresh matrix (copied on the device, untimed) and a device synchronisation per window,")
    w("# windows adding up to >= %.1f s, every case warmed; this build and the parent commit's library in processes of their own," % WINDOW)
    w("# alternating, two rounds each, the smaller mean shown.  parent = one launch per row (mat_resize_rows); vector = one")
    w("# DspVec.interpolatef over rows x points points (the ceiling); loop = get_row -> DspVec.interpolatef -> set_row on %d rows." % LOOP_ROWS)
    runs = {"tree": [], "parent": []}
    for _ in range(2):
        for name, lib in (("tree", ""), ("parent", BASELINE)):
            text = run_with(lib, [os.path.abspath(__file__), "--worker"])
            runs[name].append(json.loads(re.search(r"^RESULT (.*)$", text, re.M).group(1)))
    best = lambda name, key: min(r[key] for r in runs[name] if key in r)  # noqa: E731
    w("%-36s %10s %10s %10s %10s %9s %9s %10s" % ("rows x points, factor", "shared us", "per-row us", "parent us", "vector us",
                                                    "/ parent", "/ vector", "loop us/row"))
    for rows, points in SHAPES:
        for label, *_ in CASES:
            key = "%d x %d %s" % (rows, points, label)
            sh, pr = best("tree", key + " | shared"), best("tree", key + " | per-row")
            pa, ve, lo = best("parent", key + " | shared"), best("tree", key + " | vector"), best("tree", key + " | loop/row")
            w("%-36s %10.1f %10.1f %10.1f %10.1f %9.2f %9.2f %10.2f" % (key, sh, pr, pa, ve, sh / pa, sh / ve, lo))
    if not a.skip_vector:
        w("# the vector call, which must not pay for the row dimension: parent - tree - parent - tree, each tool's own output;")
        w("# the spread between the two parent runs is the allowance for the tree's mean")
        for tool in VECTOR_TOOLS:
            for rep in (1, 2):
                for name, lib in (("parent", BASELINE), ("tree", "")):
                    w("## %s, %s, run %d" % (tool, name, rep))
                    try:
                        text = run_with(lib, [os.path.join(ROOT, tool)])
                    except SystemExit as e:
                        text = "# did not run: %s" % str(e).splitlines()[0]
                    for line in text.splitlines():
                        if line.strip() and "amdgpu.ids" not in line:
                            w(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
