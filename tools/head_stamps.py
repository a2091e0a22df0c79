"""Where the head of the 1D step launch spends its time (profiles/r08_ab_notes.txt, step 0): a DIAGNOSTIC build of pdegym_1d.hip
(-DPDEGYM_HEAD_STAMPS) stamps the 100 MHz real-time clock three times per wave -- at wave entry, when the head's pointers are in
SGPRs, and when the row, beta and the per-instance words have arrived -- and this script prints the median over the waves of one
launch of the headline shape (parabolic nx = 256, B = 4096, S = 100).  The shipped library executes no stamp.

    python tools/head_stamps.py --build      # on the build machine: pdecontrolgym_amd/lib/ab/libstamps_{new,parent}.so
    python tools/head_stamps.py              # on the GPU: both libraries, one child process each

`new` = the kernels as the launcher picks them, `parent` = every launch through step1d_kernel (arguments inside the structures).
Each stamp holds the wave until its clock value is back (some tens of ns), so the figures are upper bounds of the undisturbed head.
"""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
AB = os.path.join(ROOT, "pdecontrolgym_amd", "lib", "ab")
VARIANTS = {"new": "1", "parent": "2"}


def build():
    from pdecontrolgym_amd import build as b
    b.build()
    os.makedirs(AB, exist_ok=True)
    hipcc = "hipcc"
    others = [os.path.join(b.LIBDIR, s.replace(".hip", ".o")) for s in b.SOURCES if s != "pdegym_1d.hip"]
    for name, val in VARIANTS.items():
        obj = os.path.join(AB, f"stamps_{name}.o")
        subprocess.run([hipcc] + b.FLAGS + b.FILE_OPTS.get("pdegym_1d.hip", []) + [f"-DPDEGYM_HEAD_STAMPS={val}", "-c",
                       os.path.join(b.CSRC, "pdegym_1d.hip"), "-o", obj], check=True)
        subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", os.path.join(AB, f"libstamps_{name}.so")] + others + [obj],
                       check=True)
        os.remove(obj)
        print(os.path.join(AB, f"libstamps_{name}.so"))


def measure(name):
    import numpy as np
    from pdecontrolgym_amd import _native as N
    N.LIB_PATH = os.path.join(AB, f"libstamps_{name}.so")
    import torch
    import bench
    wl = bench.WORKLOADS["parabolic_c2"](torch.device("cuda", 0), 1)
    wl.prepare(40)
    for _ in range(30):
        wl.step()
    torch.cuda.synchronize()
    B = 4096
    out = np.zeros(3 * B, dtype=np.uint64)
    lib = ctypes.CDLL(N.LIB_PATH)
    rc = lib.pdegym_head_stamps_read(out.ctypes.data_as(ctypes.c_void_p), B)
    assert rc == 0, rc
    t = out.reshape(B, 3).astype(np.int64)
    d1, d2 = (t[:, 1] - t[:, 0]) * 10, (t[:, 2] - t[:, 0]) * 10          # ns
    first = t[:, 0].min()
    print(f"{name:7s} entry -> pointers in SGPRs: median {np.median(d1):7.0f} ns (p10 {np.percentile(d1, 10):.0f}, p90 {np.percentile(d1, 90):.0f})"
          f" | entry -> row and beta arrived: median {np.median(d2):7.0f} ns (p10 {np.percentile(d2, 10):.0f}, p90 {np.percentile(d2, 90):.0f})"
          f" | wave entry after the launch's first wave: median {np.median(t[:, 0] - first) * 10:.0f} ns, last {(t[:, 0].max() - first) * 10} ns",
          flush=True)


if __name__ == "__main__":
    if "--build" in sys.argv:
        build()
    elif len(sys.argv) > 1:
        measure(sys.argv[1])
    else:
        for v in VARIANTS:
            r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), v])
            if r.returncode != 0:
                sys.exit(r.returncode)
