"""The launch helper on the device (kernel_lds / kernel_slots, runtime.cpp): a launcher raises the dynamic-LDS limit of
the instantiation it launches, whichever call of a process comes first.  tests/launch_order_process.py, in a child of its
own, starts with an inverse plain transform (f32, 4000 points), then a forward windowed one, then an inverse f64 one of 2000
points and a forward shifted one of 640: three register-resident lengths above 64 KiB of LDS, both directions, the option
and the plain path and, for 4000 points, the plain-only instantiation -- each held to the oracle at the bound of
test_register_resident_three_stage_batches (tests/test_gpu_parity.py), rel-L2 1e-6 (f32) / 1e-12 (f64).
A guard for the per-launch form, not a test that tells it from what came before: the launchers that raised the limit once,
behind a static, raised it for both directions on the first call and pass this order of calls as well."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def reg3_lds_bytes(radices, elem):
    """MrReg3 of mixed_radix_reg3.h: (threads per workgroup, bytes of dynamic LDS) for complex elements of 2 * elem bytes"""
    r0, r1, r2 = radices
    n = r0 * r1 * r2
    nt = n // min(radices)
    threads = 256 if nt <= 256 else 512
    la = (n // r0) * (r0 | 1)
    sb = r0 * r1 + (r0 - r0 * r1) % 32  # (Python's % is already non-negative)
    return threads, 2 * elem * (threads // nt) * (la + r2 * sb)


def test_the_first_calls_of_a_process_raise_the_limit_of_the_kernel_they_launch():
    # the three lengths take k_mr_reg3 (the table tools/gen_reg3_table.py prints is the one the header holds) with more
    # than 64 KiB of LDS, and 4000 points is a 512-thread length: f32 has its plain-only instantiation
    table = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_reg3_table.py")], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(ROOT, "basic_dsp_amd", "csrc", "mixed_radix_reg3.h")).read()
    for n, elem, threads in ((4000, 4, 512), (2000, 8, 256), (640, 8, 256)):
        m = re.search(r"BDSP_REG3\(%d, (\d+), (\d+), (\d+)\)" % n, table)
        assert m and m.group(0) in header, n
        th, lds = reg3_lds_bytes(tuple(int(g) for g in m.groups()), elem)
        assert th == threads and 64 * 1024 < lds <= 160 * 1024, (n, th, lds)
    r = subprocess.run([sys.executable, os.path.join(HERE, "launch_order_process.py")], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("ok"), r.returncode
    assert len(re.findall(r"^call \d .*rel-L2", r.stdout, re.M)) == 1 + 3 + 1 + 2
