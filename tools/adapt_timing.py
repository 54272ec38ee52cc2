#!/usr/bin/env python3
"""Timing of one tick of the adaptive signal (development aid; bench.py does not cover it; numbers: profiles/adaptation.md).

1000 neurons, 12 inputs (q, dq of six joints), 6 outputs per row; fp64 and fp32, "lif" and "lif_rate".  HIP events on the
launch stream, 3 warm-up rounds, the median of 10 timed ones; prints ONE JSON line:
  graph_us[dtype][type]    the tick at 4096 rows inside a recorded plan, launch_graph(200), per tick
  direct_us[dtype][type]   the tick at 65536 rows, 20 launches back to back, per tick
each with `hbm_fraction`: the algorithmic bytes - the per-row state read and written once; the shared tables are not
counted - over the time, as a fraction of the 8 TB/s HBM peak.

    python tools/adapt_timing.py [--rows-graph 4096] [--rows-direct 65536]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARMUP, TIMED = 3, 10
N, D, O = 1000, 12, 6
HBM_PEAK = 8e12


def row_bytes(dtype, neuron_type):
    per_neuron = 1 + O + (2 if neuron_type == "lif" else 0)  # a_f, a column of W, v and ref
    return 2 * (D + 2 * O + N * per_neuron) * np.dtype(dtype).itemsize


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-graph", type=int, default=4096)
    ap.add_argument("--rows-direct", type=int, default=65536)
    args = ap.parse_args()
    import abr_control_amd as a
    from abr_control_amd import _abi, engine

    s = a.Stream(0)
    e0, e1 = a.Event(0), a.Event(0)

    def timed(fn, per):
        for _ in range(WARMUP):
            fn()
        s.sync()
        ts = []
        for _ in range(TIMED):
            e0.record(s)
            fn()
            e1.record(s)
            s.sync()
            ts.append(e1.elapsed_ms_since(e0) * 1e3 / per)
        return {"median_us": float(np.median(ts)), "min_us": float(np.min(ts)), "max_us": float(np.max(ts))}

    rng = np.random.RandomState(0)
    enc = rng.standard_normal((N, D))
    enc /= np.linalg.norm(enc, axis=1, keepdims=True)
    gain, bias = _abi.lif_gain_bias(rng.uniform(-0.5, 0.5, N), rng.uniform(200, 400, N))
    res = {"device": a.device_name(0), "neurons": N, "inputs": D, "outputs": O, "warmup": WARMUP, "timed": TIMED,
           "rows_graph": args.rows_graph, "rows_direct": args.rows_direct, "graph_us": {}, "direct_us": {}}
    for dtype in (np.float64, np.float32):
        name = np.dtype(dtype).name
        dev = lambda x: a.DeviceArray.from_numpy(np.ascontiguousarray(x, dtype=dtype))
        tables = [dev(x) for x in (enc, gain, bias, np.zeros(D), np.ones(D))]
        for leg, B in (("graph_us", args.rows_graph), ("direct_us", args.rows_direct)):
            q, dq = dev(rng.uniform(-0.5, 0.5, (B, D // 2))), dev(rng.uniform(-0.5, 0.5, (B, D // 2)))
            ts, u = dev(rng.uniform(-30, 30, (B, O))), dev(np.zeros((B, O)))
            out = a.DeviceArray((B, O), dtype)
            for neuron_type in ("lif", "lif_rate"):
                p = _abi.make_adapt_params(D, O, N, 1, neuron_type, pes_learning_rate=1e-4)
                st = {k: a.DeviceArray(sh, dtype).zero_(s) for k, sh in engine.adapt_state_shapes(p, B).items()
                      if neuron_type == "lif" or k not in ("v", "ref")}
                step = lambda: engine.adapt_step(p, *tables, q, ts, st, in1=dq, out=out, u_add=u, dtype=dtype, stream=s)
                if leg == "graph_us":
                    with engine.Plan(device=0, stream=s) as tick:
                        step()
                    r = timed(lambda: tick.launch_graph(200), per=200)
                    tick.close()
                else:
                    def burst():
                        for _ in range(20):
                            step()
                    r = timed(burst, per=20)
                r["bytes_per_row"] = row_bytes(dtype, neuron_type)
                r["hbm_fraction"] = B * r["bytes_per_row"] / (r["median_us"] * 1e-6) / HBM_PEAK
                res[leg].setdefault(name, {})[neuron_type] = r
                for arr in st.values():
                    arr.free()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
