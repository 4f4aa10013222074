"""Cost of the source-illumination accumulation (fwi_set_illumination) per shot-gradient: forward (save) + adjoint
(image) with the accumulator off and on, alternating on one context each, at 256^3 x 1000 steps (increment form) and
at 1024^2 x 2000 steps (configs[1] / [2] grid).  Prints one JSON line per case; run it under
`rocprofv3 --kernel-trace --stats` for the illum_accumulate kernel time itself."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from full_waveform_inversion_amd import Engine, workloads  # noqa: E402


def probe(w, reps, **kw):
    wav = w.wavelet()
    src, rec = w.src_idx[:1], w.rec_idx
    with Engine(w.shape, w.h, w.dt, w.nt, order=w.order, npml=w.npml, sigma_max=0.0 if w.npml == 0 else None, **kw) as e:
        e.set_model(w.c.astype(np.float32))
        d = e.forward(None, (src, wav), rec, save=True)
        times = {False: [], True: []}
        for r in range(2 * reps + 2):
            on = bool(r % 2)
            e.set_illumination(on)
            e.synchronize()
            t0 = time.perf_counter()
            e.forward(None, (src, wav), rec, save=True)
            e.adjoint(d * 0.5)
            e.synchronize()
            if r >= 2:  # (the first pair warms up)
                times[on].append(time.perf_counter() - t0)
        off, on = float(np.median(times[False])) * 1e3, float(np.median(times[True])) * 1e3
        store_bytes = int(np.prod(w.shape)) * 4 * w.nt
        return {"config": w.name, "shape": list(w.shape), "nt": w.nt, "kernel": e.kernel_name, **kw,
                "shot_gradient_ms_off": round(off, 2), "shot_gradient_ms_on": round(on, 2),
                "added_pct": round(100.0 * (on - off) / off, 2), "store_bytes_read": store_bytes,
                "reps": reps}


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    print(json.dumps(probe(workloads.cfg4(1.0), reps, update_form="increment")), flush=True)
    print(json.dumps(probe(workloads.cfg2(1.0), reps)), flush=True)
