#!/usr/bin/env python3
"""GPU box: lifetimes of the persistent waves of dfire_bm_pairs (LIGHTDOCK_BM_DEBUG): how evenly the jobs are spread."""
import os, sys, subprocess
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["LIGHTDOCK_BM_DEBUG"] = "/tmp/bm_debug.txt"
subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "2", "--warmup", "1", "--cpu-seconds", "0"] + sys.argv[1:], check=True, stdout=subprocess.DEVNULL)
d = np.loadtxt("/tmp/bm_debug.txt")
t0, t1, jobs, batches = d[:, 0], d[:, 1], d[:, 2], d[:, 3]
start = t0.min()
life = (t1 - t0) / 100.0   # us (100 MHz)
end = (t1 - start) / 100.0
print("waves %d; kernel span %.1f us; wave lifetime mean %.1f us, min %.1f, max %.1f; last start %.1f us" % (len(d), end.max(), life.mean(), life.min(), life.max(), (t0.max() - start) / 100.0))
print("jobs per wave mean %.1f (min %d max %d); batches per wave mean %.1f (min %d, max %d); total batches %d" % (jobs.mean(), jobs.min(), jobs.max(), batches.mean(), batches.min(), batches.max(), batches.sum()))
print("us per batch (lifetime / batches): mean %.2f" % (life.sum() / batches.sum()))
h, edges = np.histogram(end, bins=10)
print("wave end-time histogram (us):", " ".join("%d@%.0f" % (c, e) for c, e in zip(h, edges[1:])))
print("time in batches: mean %.1f us per wave (%.2f us per batch); in exact-path drains %.1f us; in block set-up %.1f us; in job set-up %.1f us (%.2f us per job)" % ((d[:, 4] / 100).mean(), d[:, 4].sum() / 100 / batches.sum(), (d[:, 5] / 100).mean(), (d[:, 6] / 100).mean(), (d[:, 7] / 100).mean(), d[:, 7].sum() / 100 / max(jobs.sum(), 1)))
if d.shape[1] >= 14:   # the block set-up split (words 8-13): the rows' copy issued, the item list formed (of it: the reads' round trip), the first loads' chain; the first batch's wait
    blocks = np.maximum(d[:, 12].sum(), 1)
    us = lambda k: (d[:, k] / 100).mean()
    print("block set-ups per wave mean %.1f (%.2f us each): rows' copy issued %.1f us, item list %.1f us (its reads' round trip %.1f us), first loads' chain %.1f us per wave; first batches' wait for rows and loads %.1f us per wave (%.2f us per block)" % (
        d[:, 12].mean(), d[:, 6].sum() / 100 / blocks, us(8), us(9), us(13), us(10), us(11), d[:, 11].sum() / 100 / blocks))
if d.shape[1] >= 24:   # the drains' split (columns 14-23; the DEBUG kernel waits at the end of every phase, so a phase's time is its round trip)
    us = lambda k: (d[:, k] / 100).mean()
    drains, trips = np.maximum(d[:, 20].sum(), 1), np.maximum(d[:, 21].sum(), 1)
    print("drains per wave mean %.1f, trips %.1f (longest drain %d trips), pairs evaluated %.0f per wave (%d in all); %.2f us per trip: fence + items %.1f us, the rows' wait %.1f us, arithmetic %.1f us, the table wait %.1f us, atomics + closing fence %.1f us per wave; rechecks and the rest of the drain timer %.1f us; a drain's first trip %.2f us, a later trip %.2f us" % (
        d[:, 20].mean(), d[:, 21].mean(), d[:, 23].max(), d[:, 22].mean(), d[:, 22].sum(), d[:, 14:19].sum() / 100 / trips, us(14), us(15), us(16), us(17), us(18),
        (d[:, 5] / 100).mean() - (d[:, 14:19].sum(1) / 100).mean(), d[:, 19].sum() / 100 / drains,
        (d[:, 14:19].sum() - d[:, 19].sum()) / 100 / np.maximum(trips - drains, 1)))
if d.shape[1] >= 27:   # bm_recheck (columns 24-26): the blocks with several flagged pairs, their pairs found again
    print("bm_recheck: %.1f us per wave in %.1f rounds of 64 (entry, block) items at most (%.2f us a round), %.0f items per wave" % (
        (d[:, 24] / 100).mean(), d[:, 25].mean(), d[:, 24].sum() / 100 / np.maximum(d[:, 25].sum(), 1), d[:, 26].mean()))
late = end > np.percentile(end, 90)
print("slowest 10%% of waves: batches %.0f, batch time %.0f us, drain time %.0f us, jobs %.1f" % (batches[late].mean(), (d[late, 4] / 100).mean(), (d[late, 5] / 100).mean(), jobs[late].mean()))
per_cu = batches.reshape(-1, 8).sum(1)
print("batches per CU: mean %.0f min %d max %d" % (per_cu.mean(), per_cu.min(), per_cu.max()))
