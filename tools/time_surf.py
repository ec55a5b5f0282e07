"""svs_surf_extract at the keyframe size (640 x 480, the reference's parameters) for 1, 8 and 64 images: per-stage device time from the library's own events
(svs_surf_stage_times), the wall time of the blocking call, and for the integral and response stages the achieved fraction of HBM peak against their
algorithmic bytes.  The yardstick is the work the call replaces, measured here too: the download of an image and its disparity plus the
upload of the place through svs_loop_set_place; the NumPy restatement's time on one image is given as context only.  Also the band statistics of the test
images of tests/test_gpu_surf.py (model alone).
usage: python tools/time_surf.py [out.md]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch

import surf_model as M
from scavislam_amd import capi
from scavislam_amd.loop import GeometricChecker, SurfExtractor

W, H, REPS = 640, 480, 15
HBM_PEAK = 8.0e12      # bytes / s, spec (MI355X)
CAM = dict(f=570.342, cx=320.0, cy=240.0, b=0.075)
args = [a for a in sys.argv[1:] if not a.startswith("--")]

base = [M.blob_image(W, H, 10 + k, n_blobs=1500) for k in range(4)]
disp1 = np.full((H, W), 14.0, np.float32)
ctx = capi.Context(0)
out = ["svs_surf_extract, 640 x 480 u8 images + f32 disparity, SurfFeatureDetector(600, 2) / SurfDescriptorExtractor(2, 4, 2, false) (1 x MI355X; stage times from "
       f"events, medians of {REPS} calls after 3 warm-up calls; clocks as the machine had them, not pinned).", "",
       "| images | keypoints / image | integral (ms) | responses (ms) | maxima (ms) | order (ms) | orientation + descriptor (ms) | compaction (ms) | stages total (ms) | wall (ms) | wall / image (ms) | integral: share of HBM peak | responses: share of HBM peak |",
       "|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|"]
planes = sum(((H >> o) * (W >> o)) * 4 for o in range(2))                 # elements of the 8 planes of one image
for nb in (1, 8, 64):
    imgs = np.stack([base[k % 4] for k in range(nb)])
    d_img = torch.as_tensor(imgs).cuda()
    d_disp = torch.as_tensor(np.broadcast_to(disp1, (nb, H, W)).copy()).cuda()
    torch.cuda.synchronize()
    ex = SurfExtractor(ctx, CAM, W, H, max_batch=nb, max_keypoints=2048)
    ex.set_timing(True)
    st, wall = [], []
    for r in range(REPS + 3):
        pl = ex.extract_device(d_img.data_ptr(), W, W * H, d_disp.data_ptr(), W, W * H, nb)
        if r >= 3:
            st.append(ex.stage_times_ms()), wall.append(ex.last_call_ms)
    ms = [statistics.median(s[i] for s in st) for i in range(6)]
    wl = statistics.median(wall)
    nkp = sum(len(p) for p in pl) / nb
    b_int = nb * (W * H * 1 + (W + 1) * (H + 1) * 4 * 3)                  # read the image; write the row sums, read and write them in the column pass
    b_rsp = nb * ((W + 1) * (H + 1) * 4 + planes * 4 * 2 * 2)             # read the integral image once; zero and write det and trace
    out.append(f"| {nb} | {nkp:.0f} | {ms[0]:.3f} | {ms[1]:.3f} | {ms[2]:.3f} | {ms[3]:.3f} | {ms[4]:.3f} | {ms[5]:.3f} | {sum(ms):.3f} | {wl:.3f} | {wl / nb:.3f} | "
               f"{b_int / (ms[0] * 1e-3) / HBM_PEAK:.1%} | {b_rsp / (ms[1] * 1e-3) / HBM_PEAK:.1%} |")
    print(out[-1], flush=True)
    if nb == 1:
        # what the call replaces: image + disparity down, the place up through svs_loop_set_place
        gc = GeometricChecker(ctx, CAM, max_desc=2048, max_places=2)
        h_img, h_disp = torch.empty((H, W), dtype=torch.uint8).pin_memory(), torch.empty((H, W), dtype=torch.float32).pin_memory()
        down, up, dev = [], [], []
        for r in range(REPS + 3):
            t0 = time.perf_counter()
            h_img.copy_(d_img[0]), h_disp.copy_(d_disp[0])
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            gc.set_place(0, pl[0].descriptors, pl[0].uvu)
            ctx.sync()
            t2 = time.perf_counter()
            gc.set_place_from_surf(1, ex, 0)
            ctx.sync()
            t3 = time.perf_counter()
            if r >= 3:
                down.append((t1 - t0) * 1e3), up.append((t2 - t1) * 1e3), dev.append((t3 - t2) * 1e3)
        t0 = time.perf_counter()
        m = M.extract(base[0], disp1)
        model_s = time.perf_counter() - t0
        round_trip = (f"The round trip the call replaces, one image: download of the image and its disparity {statistics.median(down):.3f} ms, upload of the place "
                      f"({len(pl[0])} descriptors) through svs_loop_set_place {statistics.median(up):.3f} ms (wall, synchronised) -- the description itself would come on top, "
                      f"on a host library the ROCm side does not have.  svs_loop_set_place_from_surf instead: {statistics.median(dev):.3f} ms.  For context only: the NumPy "
                      f"restatement takes {model_s:.1f} s on this image on the host ({len(m['kp'])} keypoints).")
        gc.close()
    ex.close()
ctx.close()
out += ["", round_trip, "",
        "Algorithmic bytes: integral = image read + 3 x the int32 integral image (row sums written, column pass reads and writes); responses = integral image read once + "
        "det and trace planes zeroed and written.  A stage far below the peak at these sizes is bound by launches and latency (one image is 0.3 MB of pixels), not by bytes.",
        "", "Band statistics of the test images (tests/surf_model.py alone; a keypoint in a band is held to the weaker check of tests/test_gpu_surf.py):", "",
        "| image | keypoints | maxima | in bands |", "|---|---:|---:|---:|"]
for name, (w, h, seed, nbl, sg) in M.TEST_IMAGES.items():
    m = M.extract(*M.test_image(name))
    out.append(f"| {w} x {h}, seed {seed} | {len(m['kp'])} | {m['n_maxima']} | {int(m['band'].sum())} |")
out += ["", "Rotation by 90 degrees on the model (tests/test_surf_cpu.py, 140 x 140, seed 3): worst position difference 7.6e-6 px, angles exactly 90 degrees apart, "
        "worst descriptor distance 1.3e-4."]
text = "\n".join(out)
print(text)
if args:
    os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
    open(args[0], "w").write(text + "\n")
