"""Per-wave phase stamps of the main k-NN launch for any k / method (dev tool; needs a library
built with -DPTV_STAMP_ALL=1 for KMAX != 8, e.g. PTV_LIB=ab/libptv_stamp.so).

usage: stamp_k.py [--xcd [--chunks C0,C1,...]] G N k [idw|sibson|filter]   (filter: PTV_STAMP_LATTICE=4 is set here)

--xcd: how the launch's waves spread over the XCDs, from each wave's XCD id and its first and last
value of the device's real-time clock (100 MHz): per XCD the waves, their summed time, the first
start, the last start (the XCD has no block left to take) and the last end; for the launch the
span, the first XCD out of work, the spread of the XCDs' ends and the tail after 99 % of the waves.
--chunks: one stamped launch and table per chunk length of the XCD map, in blocks (0 = one contiguous
range per XCD, -1 = the launcher's own).  The stamped build is slower than the real one: read the
shares, not the milliseconds.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ptv_interpolation_amd import _lib, synth

argv = sys.argv[1:]
xcd = "--xcd" in argv
chunks = [-1]
if "--chunks" in argv:
    i = argv.index("--chunks")
    chunks = [int(v) for v in argv[i + 1].split(",")]
    del argv[i:i + 2]
argv = [a for a in argv if a != "--xcd"]
G, N, k = (int(v) for v in argv[:3])
method = argv[3] if len(argv) > 3 else "idw"
m = _lib.METHOD_IDW if method == "idw" else _lib.METHOD_SIBSON
if method == "filter":
    os.environ["PTV_STAMP_LATTICE"] = "4"
P, Q = synth.sphere_pack(N, G)
ax = np.linspace(0, G - 1, G)
ctx = _lib.Context.get(0)


def xcd_table(x, chunk):
    """x: (waves, 3) uint64 {XCD, first, last real-time clock} in dispatch order."""
    slot = (np.arange(len(x)) >> 2) & 7  # the wave's block's dispatch slot class (block % 8)
    ok = x[:, 2] > 0
    x, slot = x[ok], slot[ok]
    xc = x[:, 0].astype(np.int64)
    t0 = int(x[:, 1].min())
    a = (x[:, 1].astype(np.int64) - t0) * 1e-5  # ms at 100 MHz
    e = (x[:, 2].astype(np.int64) - t0) * 1e-5
    span = e.max()
    print(f"   xcd table: {len(x)} waves, chunk {chunk} blocks" + (" (the launcher's own)" if chunk < 0 else ""))
    print("   xcd   waves  wave-ms(sum)  share   first-start  last-start  last-end   slot classes (block % 8) seen")
    ends, outs = [], []
    tot = (e - a).sum()
    for d in sorted(set(xc.tolist())):
        s = xc == d
        ends.append(e[s].max())
        outs.append(a[s].max())
        cls = ",".join(str(v) for v in sorted(set(slot[s].tolist())))
        print(f"   {d:3d} {s.sum():8d} {(e[s] - a[s]).sum():12.1f} {100 * (e[s] - a[s]).sum() / tot:6.2f}% "
              f"{a[s].min():11.4f} {a[s].max():11.4f} {e[s].max():9.4f}   {cls}")
    es = np.sort(e)
    p99 = es[int(0.99 * (len(es) - 1))]
    print(f"   launch: span {span:.4f} ms; first XCD out of work at {min(outs):.4f} ms ({100 * min(outs) / span:.1f} % of the span); "
          f"XCD ends {min(ends):.4f} .. {max(ends):.4f}, spread {max(ends) - min(ends):.4f} ms ({100 * (max(ends) - min(ends)) / span:.2f} %); "
          f"XCD last starts spread {max(outs) - min(outs):.4f} ms ({100 * (max(outs) - min(outs)) / span:.2f} %)")
    print(f"   tail: 99 % of the waves done at {p99:.4f} ms, last end {span:.4f}: {span - p99:.4f} ms ({100 * (span - p99) / span:.2f} %)")
    d = e - a
    ds = np.sort(d)
    print(f"   wave time: mean {d.mean() * 1e3:.1f} us, p50 {ds[len(ds) // 2] * 1e3:.1f}, p99 {ds[int(0.99 * (len(ds) - 1))] * 1e3:.1f}, "
          f"p99.9 {ds[int(0.999 * (len(ds) - 1))] * 1e3:.1f}, max {ds[-1] * 1e3:.1f}; waves in flight on average {tot / span:.0f}", flush=True)


def run(chunk):
    _lib.debug_xcd_chunk(chunk)
    for it in range(2):
        if it == 1:
            ctx.debug_stamps(1)
        if method == "filter":
            ctx.filter_outliers_knn(P, Q, k=k)
        else:
            ctx.interp_knn(P, Q, axes=(ax, ax, ax), method=m, k=k)
    st = ctx.stats
    c = ctx.debug_stamps(2)
    x = ctx.debug_xcd_stamps() if xcd else None
    ctx.debug_stamps(0)
    print(f"{method} k={k} G={G} N={N}: lat {st.get('ms_lattice', 0):.2f} knn {st.get('ms_knn', 0):.2f} ms, waves {c['waves']:.0f}")
    print("   mean per wave:", {k2: round(v, 1) for k2, v in c["mean"].items()})
    print("   max per wave: ", {k2: round(v, 1) for k2, v in c["max"].items()}, flush=True)
    if xcd:
        xcd_table(x, chunk)


for chunk in chunks:
    run(chunk)
_lib.debug_xcd_chunk(-1)
