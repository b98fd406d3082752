"""Phase clocks of the two-sided solve's wavefronts in the headline's grouped dispatch.  Needs the experiment build
  python -m mrs_uav_trajectory_generation_amd.build --variant stamps -DMRS_TG_DUO_STAMPS=1
and MRS_TG_LIB_PATH pointing at libmrs_tg_stamps.so; runs bench.py's headline in this process, then reads the stamps of the last
dispatches (mrs_tg_debug_duo_stamps) and prints the mean / median clocks between the stamps (s_memtime: the shader clock, one
counter per XCD -- differences within a wavefront only), and from the device-wide 100 MHz clock (s_memrealtime) at a wavefront's
entry and behind its final wait: shader clocks per microsecond, and first entry -> last exit of each dispatch in microseconds
(the headline's two dispatches run side by side and share the rows: a row belongs to the dispatch that wrote it last).
  MRS_TG_LIB_PATH=$PWD/mrs_uav_trajectory_generation_amd/libmrs_tg_stamps.so python scripts/duo_phase_clocks.py"""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.argv = ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "3", "--no-cpu-baseline", "--no-extras"] + sys.argv[1:]
import bench
try:
    bench.main()
except SystemExit:
    pass
from mrs_uav_trajectory_generation_amd import api
L = api.load_library()
SLOTS = 20   # kDuoStampSlots: 0 .. 13 shader clock, 14 / 15 device-wide clock at entry / exit, 16 the dispatch's tag
buf = (C.c_ulonglong * (2048 * SLOTS))()
rc = L.mrs_tg_debug_duo_stamps(buf)
a = np.frombuffer(buf, dtype=np.uint64).reshape(2048, SLOTS).astype(np.int64)
a = a[a[:, 0] != 0]
order = [0, 1, 13, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12]
# two wavefronts of the two dispatches with one workgroup index may have written a row at the same time: such a row's stamps are
# not in order (or its life is not a wavefront's), and it is left out
n_rows = len(a)
steps_ok = np.all(np.diff(a[:, order], axis=1) >= 0, axis=1) & (a[:, 12] - a[:, 0] < 1000000)
real_ok = (a[:, 15] > a[:, 14]) & (a[:, 15] - a[:, 14] < 100000)
a = a[steps_ok & real_ok]
print("rc", rc, "wavefronts with stamps", n_rows, "of which rows written by one wavefront", len(a))
names = {1: "entry -> path index known (kernel arguments)", 13: "-> loads of the first trip issued", 2: "-> loads arrived, LDS written, end checks",
         3: "-> ballots, LDS fence", 4: "-> constants, longest side: before the forward loop", 5: "-> forward step 0", 6: "-> forward step 1",
         7: "-> forward steps 2..", 8: "-> join", 9: "-> first backward step", 10: "-> other backward steps", 11: "-> cost / status issued",
         12: "-> stores acknowledged"}
tot = a[:, 12] - a[:, 0]
print("wavefront life: mean %.0f  median %.0f  min %d  max %d clocks" % (tot.mean(), np.median(tot), tot.min(), tot.max()))
for k0, k1 in zip(order[:-1], order[1:]):
    d = a[:, k1] - a[:, k0]
    print("  %-55s mean %8.0f  median %8.0f  (%.1f %%)" % (names[k1], d.mean(), np.median(d), 100 * d.mean() / tot.mean()))
# the device-wide clock: 100 MHz, so 100 ticks per microsecond
life_us = (a[:, 15] - a[:, 14]) / 100.0
mhz = tot[life_us > 0] / life_us[life_us > 0]
print("shader clock: median %.0f MHz (min %.0f, max %.0f) = clocks of a wavefront's life / its microseconds" % (np.median(mhz), mhz.min(), mhz.max()))
print("wavefront life: median %.2f us  max %.2f us  (max / median %.2f)" % (np.median(life_us), life_us.max(), life_us.max() / np.median(life_us)))
for tag in sorted(set(a[:, 16])):
    w = a[a[:, 16] == tag]
    if len(w) < 64:   # (the other dispatch's rows that were not overwritten: too few for a span)
        print("dispatch %#x: %4d wavefronts (rows the later dispatch did not overwrite)" % (tag, len(w)))
        continue
    first, last = w[:, 14].min(), w[:, 15].max()
    print("dispatch %#x: %4d wavefronts, first entry -> last exit %.2f us, first -> last entry %.2f us, first -> last exit %.2f us"
          % (tag, len(w), (last - first) / 100.0, (w[:, 14].max() - first) / 100.0, (last - w[:, 15].min()) / 100.0))
t0 = a[:, 14].min()
print("both dispatches: first entry -> last exit %.2f us" % ((a[:, 15].max() - t0) / 100.0))
