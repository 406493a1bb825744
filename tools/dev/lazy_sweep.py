"""dev: lazy_top 0 against 1, whole calls, on 4096^2 frames of graded keypoint density (DESIGN_APPENDIX part L-3; run from the
repository root: python tools/dev/lazy_sweep.py; raw output of the recorded run: profiles/lazy_top/density_sweep.txt)"""
import sys, os, time, json
sys.path.insert(0, os.getcwd())
import numpy as np, torch
from scipy.ndimage import gaussian_filter
import sift_pyocl_amd as sp

size = 4096
frames = [("white", np.random.default_rng(1).random((size, size), dtype=np.float32), 3)]
for sg in (1.0, 2.0, 3.0):
    frames.append(("sigma%g" % sg, gaussian_filter(np.random.default_rng(3).random((size, size)), sg).astype(np.float32), 3 if sg < 3 else None))
for name, img, octs in frames:
    t = torch.from_numpy(img).cuda()
    plans = {}
    for mode in (0, 1):
        p = sp.SiftPlan(shape=(size, size), dtype=np.float32, devicetype="GPU", device=0, octave_max=octs)
        p.set_option("lazy_top", mode)
        for _ in range(8):
            kp = p.keypoints(t)
        plans[mode] = p
    cs = plans[0].last_counts()["c_scale"]
    res = {0: [], 1: []}
    for rnd in range(5):
        for mode in (0, 1):
            p = plans[mode]
            for _ in range(3):
                p.keypoints(t)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(15):
                p.keypoints(t)
            res[mode].append((time.perf_counter() - t1) / 15 * 1e3)
    px = [(size >> o) ** 2 for o in range(len(cs))]
    print(json.dumps({"frame": name, "keypoints": int(len(kp)), "scale3": cs[:, 2].tolist()[:3],
                      "pixels_per_scale3": [round(px[o] / max(1, int(cs[o, 2])), 1) for o in range(min(3, len(cs)))],
                      "eager_ms": [round(v, 4) for v in res[0]], "lazy_ms": [round(v, 4) for v in res[1]],
                      "eager_med": round(float(np.median(res[0])), 4), "lazy_med": round(float(np.median(res[1])), 4)}), flush=True)
    del plans, t
