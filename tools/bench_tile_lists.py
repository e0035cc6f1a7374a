#!/usr/bin/env python3
"""What the tile lists cost a camera that never stands still: one 1-spp frame with the camera moved before every frame, against the
same frames under FLAG_NO_TILE_LISTS, and the builder's own device time.

    python tools/bench_tile_lists.py [--frames 30] [--bounces 8]       # one JSON line

The shipped library builds the table only before the second batch a camera has been kept for, so here it never builds (builds = 0) and
only clears the table; a tuning build with -DWFPT_TILE_LISTS_EAGER=1 (tools/build_variant.sh, selected with WFPT_LIB) rebuilds it for
every frame: that pair is the measurement behind the deferral (profiles/r06_tile_lists_ab.txt).

Per size (400x225 and 1920x1080): wall milliseconds per frame (camera update + render + synchronize), median and the spread
(max - min of the per-third medians) of each arm, and the builder's event-pair time. Run on the GPU box, from the repo root."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
try:
    import torch  # noqa: F401  (before libwfpt.so: one HIP runtime per process, see tests/conftest.py)
except ImportError:
    pass
import wavefront_path_tracer_amd as W  # noqa: E402


def frames_ms(w, h, flags, frames, bounces):
    cc = W.CameraController(W.Camera.book_one_final_camera(), 20.0, 0.6, 10.0, 0.1, 100.0, 4.0, 0.1)
    rp = W.RenderParameters(cc, (w, h))
    pt = W.PathTracer(W.Scene.book_one_final(1), rp, max_wavefronts=bounces, flags=flags, batch=1)
    ms, build_ms = [], []
    for k in range(frames + 3):
        cc = rp.camera_controller().copy()
        cc.process_mouse((1.0 if k % 2 else -1.0, 0.25))  # a small turn, back and forth
        cc.update_camera(1.0 / 60.0)
        rp.update_camera_controller(cc)
        pt.synchronize()
        t0 = time.perf_counter()
        pt.update_render_parameters(rp)
        pt.update_buffers()
        pt.render(1)
        pt.synchronize()
        if k >= 3:  # (the first frames capture the graph and warm the caches)
            ms.append((time.perf_counter() - t0) * 1e3)
            if not flags & W.FLAG_NO_TILE_LISTS and pt.tile_lists_timing()[1] > 0:
                build_ms.append(pt.tile_lists_timing()[0])
    builds = 0 if flags & W.FLAG_NO_TILE_LISTS else pt.tile_lists_timing()[1]
    pt.close()
    thirds = [float(np.median(c)) for c in np.array_split(np.array(ms), 3)]
    out = {"median_ms": round(float(np.median(ms)), 4), "spread_ms": round(max(thirds) - min(thirds), 4), "builds": builds}
    if build_ms:
        out["builder_ms"] = round(float(np.median(build_ms)), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--bounces", type=int, default=8)
    a = ap.parse_args()
    out = {"library": os.environ.get("WFPT_LIB", "default"), "frames": a.frames}
    for w, h in ((400, 225), (1920, 1080)):
        out[f"{w}x{h}"] = {"lists": frames_ms(w, h, 0, a.frames, a.bounces), "walk": frames_ms(w, h, W.FLAG_NO_TILE_LISTS, a.frames, a.bounces)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
