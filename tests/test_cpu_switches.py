"""The NIDT_* environment switches the HIP sources read: conv3d.hip keeps exactly the twelve that choose between two
surviving kernels or move a live threshold (the table of the README), and no switch is read with two defaults.

The scan sees reads written as ``env_int("NIDT_...", <integer literal>)`` / ``env_int64(...)``, the one form the kernel
files use (common.h); a read with another default expression, or a kernel file calling getenv itself, fails the scan
instead of escaping it."""
import os
import re

KDIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "kernels")
READ = re.compile(r'env_int(?:64)?\("(NIDT_\w+)",\s*(-?\d+)\)')

CONV3D = {
    "NIDT_FWD_KSPLIT": 0, "NIDT_FWDG_KSPLIT": 0, "NIDT_FWD_BP_THRESH": 256, "NIDT_FWD_BP128": 1,
    "NIDT_FWD_TRI": 1, "NIDT_FWD_SLAB": 2, "NIDT_2D_SLAB": 1, "NIDT_2D_SLAB_BD": 1,
    "NIDT_WG1X1": 1, "NIDT_WG_TRI": 1, "NIDT_WG_TRI_MINPOS": 8192, "NIDT_WG_DIRECT": 1,
}


def _reads():
    out = {}
    for f in sorted(os.listdir(KDIR)):
        if f.endswith((".hip", ".h")):
            with open(os.path.join(KDIR, f)) as fh:
                src = fh.read()
            out[f] = [(n, int(d)) for n, d in READ.findall(src)]
            assert len(out[f]) == len(re.findall(r'env_int(?:64)?\(', src)) - 2 * (f == "common.h"), f
            assert ("getenv" in src) == (f == "common.h"), f  # env_int / env_int64 are the only readers
    return out


def test_conv3d_switches_are_the_kept_table():
    assert dict(_reads()["conv3d.hip"]) == CONV3D


def test_no_switch_has_two_defaults():
    seen = {}
    for f, reads in _reads().items():
        for name, dflt in reads:
            assert seen.setdefault(name, dflt) == dflt, (f, name)
    assert len(seen) > len(CONV3D)  # the scan also saw the switches of the other kernel files
