"""The groupBy sort alone (dg_debug_probe DG_PROBE_SORT): N packed words of the headline's key shape,
sorted by the engine's radix passes and checked ascending; prints ms per sort and the HBM rate of the
passes' algorithmic bytes (first-pass histogram read + per pass 8 B read + 8 B written per word), for the
classic sort and with the low 2 and 10 key bits left out (DG_PROBE_SORT_DEFER: five 7-bit, four 8-bit and
three 8-bit passes; the check is then on the sorted prefix).
usage: python tools/sort_probe.py [N] [ITERS] [D ...]   (DRUID_AMD_LIB selects a variant build)"""
import ctypes
import importlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NAT = importlib.import_module("incubator-druid_amd._native")

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 10
defers = [int(a) for a in sys.argv[3:]] or [0, 2, 10]
L = NAT.lib()
for d in defers:
    os.environ["DG_PROBE_SORT_DEFER"] = str(d)
    ms = ctypes.c_double()
    NAT.check(L.dg_debug_probe(0, 5, n, iters, ctypes.byref(ms)))
    passes = (34 - d + 7) // 8
    gb = n * (8 + 16 * passes) / 1e9
    print(f"sort {n} words, key bits [{d}, 34), {passes} passes: {ms.value:.3f} ms  "
          f"({gb / (ms.value / 1e3):.0f} GB/s of {gb:.2f} GB algorithmic)", os.environ.get("DRUID_AMD_LIB", "default"))
