"""What the per-device launch helper (kernel_lds / kernel_slots, runtime.cpp) costs a call, against a build of the parent
commit on the same MI355X in the same session -> profiles/launch_helper.txt.

  python tools/launch_helper_bench.py --parent-lib /path/to/the/parent/libbasic_dsp_hip.so --out profiles/launch_helper.txt

The driver starts one fresh process per measurement and alternates the two libraries (parent, branch, parent, branch), each
child loading the one BDSP_HIP_LIBRARY names; it never touches the device itself.  Two processes of ONE library differ by
up to 0.6 us per call (the control in profiles/launch_helper.txt), more than the helper costs: read a single pair with care.
A child measures the HOST wall time of one call of bdsp_hip_dev_fft for a batch-1 plain forward transform on the library's
own stream,

  f32 4000 points   k_mr_reg3 plain-only, 65 920 bytes of LDS: kernel_slots and kernel_lds above 64 KiB
  f32 1000 points   k_mr_reg3, 34 560 bytes: kernel_slots below 64 KiB

as the median of 3 x 2000 calls after 300 warm-up calls, every call timed on its own and one synchronise at the end of each
2000.  Between two timed calls an untimed scale by 1 / sqrt(n) on the same stream keeps the data finite (a transform
multiplies the norm by sqrt(n)).  Then bench.py --gpus 1 --steps 200 --warmup 20 with each library, in the same alternation:
its value.

The parent is measured twice: spread = |run 1 - run 2|.  The branch passes a figure when each of its medians is no worse
than the parent's worse run plus that spread (times: no larger; bench.py's value, a rate: no smaller)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = (("f32_4000", 4000), ("f32_1000", 1000))
ROUNDS, CALLS, WARM = 3, 2000, 300


def child():
    sys.path.insert(0, ROOT)
    import numpy as np
    import basic_dsp_amd as bd
    L = bd._lib
    bd.require_gpu()
    out = {"lib": L.LIB_PATH}
    for name, n in CASES:
        rng = np.random.default_rng(n)
        m = bd.DspMat(rng.uniform(-10, 10, (1, 2 * n)).astype(np.float32), is_complex=True)
        scr = bd.DspMat(np.zeros((1, 2 * n), np.float32), is_complex=True)
        d, s, flag, keep = C.c_void_p(m.device_ptr()), C.c_void_p(scr.device_ptr()), C.c_int(0), float(1.0 / np.sqrt(n))
        fft, clock = L.lib.bdsp_hip_dev_fft, time.perf_counter_ns
        ref = C.byref(flag)

        def run(calls):
            t = np.empty(calls)
            for i in range(calls):
                t0 = clock()
                code = fft(0, d, s, n, 1, 0, 1.0, -1, 0.0, ref, None)
                t[i] = clock() - t0
                assert code == 0 and flag.value == 0, (code, flag.value, L.last_error())
                assert m.scale(keep) == 0
            L.check(L.lib.bdsp_hip_synchronize(None), "synchronize")
            return t
        run(WARM)
        rounds = [run(CALLS) for _ in range(ROUNDS)]
        assert np.isfinite(m.data()).all() and np.abs(m.data()).max() > 0  # (the timed calls ran on finite, non-zero data)
        out[name] = {"median_us": float(np.median(np.concatenate(rounds))) / 1e3,
                     "round_medians_us": [float(np.median(r)) / 1e3 for r in rounds]}
    print("LAUNCH_HELPER " + json.dumps(out))


def measure(lib, what, log):
    env = dict(os.environ, BDSP_HIP_LIBRARY=lib)
    if what == "calls":
        cmd, limit = [sys.executable, os.path.abspath(__file__), "--child"], 180
    else:
        cmd, limit = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "200", "--warmup", "20"], 420
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=limit, cwd=ROOT)
    if r.returncode != 0:
        log("FAILED (%d): %s\n%s" % (r.returncode, " ".join(cmd), (r.stdout + r.stderr)[-3000:]))
        sys.exit(1)  # (nothing more is started on the device after a failure)
    if what == "calls":
        line = [l for l in r.stdout.splitlines() if l.startswith("LAUNCH_HELPER ")][-1]
        return json.loads(line[len("LAUNCH_HELPER "):])
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("{") and '"value"' in l][-1])
    return {"value": rec["value"], "unit": rec.get("unit")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--branch-lib", default=os.path.join(ROOT, "basic_dsp_amd", "lib", "libbasic_dsp_hip.so"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-bench", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child()
    lines = []

    def log(text):
        print(text, flush=True)
        lines.append(text)
    log("# python tools/launch_helper_bench.py --parent-lib %s --branch-lib %s%s%s" % (
        os.path.relpath(args.parent_lib, ROOT), os.path.relpath(args.branch_lib, ROOT), " --no-bench" if args.no_bench else "",
        " --out " + args.out if args.out else ""))
    log("# host wall time of one bdsp_hip_dev_fft call (batch 1, plain, forward), us: median of %d x %d calls; rounds in brackets" % (ROUNDS, CALLS))
    order = (("parent", args.parent_lib), ("branch", args.branch_lib)) * 2
    calls = {"parent": [], "branch": []}
    for who, lib in order:
        rec = measure(lib, "calls", log)
        calls[who].append(rec)
        log("%-6s run %d  " % (who, len(calls[who])) + "   ".join(
            "%s %.3f [%s]" % (name, rec[name]["median_us"], " ".join("%.3f" % v for v in rec[name]["round_medians_us"])) for name, _ in CASES))
    verdicts = []
    for name, _ in CASES:
        p = [r[name]["median_us"] for r in calls["parent"]]
        b = [r[name]["median_us"] for r in calls["branch"]]
        spread, bound = abs(p[0] - p[1]), max(p) + abs(p[0] - p[1])
        verdicts.append("%s: parent %.3f / %.3f us (spread %.3f), bound %.3f, branch %.3f / %.3f us: %s" % (
            name, p[0], p[1], spread, bound, b[0], b[1], "pass" if max(b) <= bound else "MISS"))
    if not args.no_bench:
        log("# bench.py --gpus 1 --steps 200 --warmup 20: value")
        bench = {"parent": [], "branch": []}
        for who, lib in order:
            rec = measure(lib, "bench", log)
            bench[who].append(rec)
            log("%-6s run %d  value %.1f %s" % (who, len(bench[who]), rec["value"], rec["unit"] or ""))
        p, b = [r["value"] for r in bench["parent"]], [r["value"] for r in bench["branch"]]
        spread, bound = abs(p[0] - p[1]), min(p) - abs(p[0] - p[1])
        verdicts.append("bench.py value: parent %.1f / %.1f (spread %.1f), bound %.1f, branch %.1f / %.1f: %s" % (
            p[0], p[1], spread, bound, b[0], b[1], "pass" if min(b) >= bound else "MISS"))
    log("# the branch passes when each of its medians is no worse than the parent's worse run plus the parent's spread")
    for v in verdicts:
        log(v)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
