"""Camera models: what the ray launches of csrc/rays_cam.hip cost beside the plain ones.  One GPU, one JSON document
(profiles/camera_bench.json unless --out says otherwise).  There is no pass mark: the yardstick is the plain launch of the same run.

Two sizes, each back to back in one process: a ray batch of 32,768 rays x 64 samples drawn over 21 views of 128 x 96 pixels, and two
whole views of 256 x 256 pixels x 64 samples.  Per size the variants in turn, --repeats rounds of --launches launches on preallocated
outputs between device events, Philox jitter (no noise array is read):
  plain          knerf_draw_ray_batch / knerf_generate_rays
  cam_plain      the new launch with the plain camera (fx = fy = focal, centred principal point, offset 0): the same bits
  cam_intrinsics pinhole with fx != fy, an off-centre principal point and pixel_offset 0.5
  cam_opencv     radial + tangential distortion: 8 Newton steps by the thread of sample 0 of every ray
  cam_fisheye    equidistant fisheye: 8 one-dimensional steps, then sin / cos
  cam_opencv_ndc distortion under NDC rays: every sample thread repeats the solve, because each needs the ray's NDC length
  ext_ndc        knerf_*_ext with NDC rays and the plain camera, what cam_opencv_ndc adds the solve to
Reported per variant: the median and the spread (min, max) over the rounds, microseconds per launch.

    python tools/camera_bench.py [--launches 2000] [--repeats 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, V, FOCAL, RAYS, N = 128, 96, 21, 120.0, 32768, 64
VIEW, VIEWS = 256, 2


def cameras(width, height, focal):
    """the camera of each variant at a width x height image; every one passes check_invertible"""
    from keras_nerf_amd.data.cameras import CameraModel
    fx, fy, cx, cy = focal, focal * 0.97, width * 0.515, height * 0.47
    out = {"cam_plain": CameraModel.from_focal(focal, width, height),
           "cam_intrinsics": CameraModel("pinhole", fx, fy, cx, cy, pixel_offset=0.5),
           "cam_opencv": CameraModel("opencv", fx, fy, cx, cy, (-0.12, 0.03, 0.002, -0.003, -0.004), pixel_offset=0.5),
           "cam_fisheye": CameraModel("fisheye", focal * 0.5, focal * 0.49, cx, cy, (-0.04, 0.01, -0.003, 0.0005), pixel_offset=0.5)}
    out["cam_opencv_ndc"] = out["cam_opencv"]
    for cam in out.values():
        cam.check_invertible(width, height)
    return out


def time_launches(n_launches, repeats):
    import numpy as np
    import torch
    from keras_nerf_amd import _lib
    from tools.forward_facing_bench import camera_poses
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(0)
    images = torch.rand((V, H, W, 4), device="cuda", generator=g)
    c2w = torch.as_tensor(camera_poses()[:V].astype(np.float32), device="cuda")
    n_out = max(RAYS, VIEWS * VIEW * VIEW)
    o = torch.empty((n_out, 3), device="cuda"); d = torch.empty_like(o); tg = torch.empty_like(o); t = torch.empty((n_out, N), device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ndc = _lib.KnerfRayModel(1, 0, 1.0)
    batch_cams, view_cams = cameras(W, H, FOCAL), cameras(VIEW, VIEW, FOCAL * 2)
    tables = {id(c): c.device_table() for c in list(batch_cams.values()) + list(view_cams.values())}

    def batch(name, k):
        near, far = (0.0, 1.0) if name.endswith("ndc") else (2.0, 6.0)
        head, tail = (None, stream, p(images), p(c2w), V, H, W, 4), (near, far, N, 1, 0, 0, RAYS, None, k, p(o), p(d), p(t), p(tg), None)
        if name == "plain":
            return lib.knerf_draw_ray_batch(*head, FOCAL, *tail)
        if name == "ext_ndc":
            return lib.knerf_draw_ray_batch_ext(*head, FOCAL, *tail, C.byref(ndc))
        cam = batch_cams[name]
        cs = cam.c_struct()
        return lib.knerf_draw_ray_batch_cam(*head, p(tables[id(cam)]), 1, C.byref(cs), *tail, C.byref(ndc) if name.endswith("ndc") else None)

    def views(name, k):
        near, far = (0.0, 1.0) if name.endswith("ndc") else (2.0, 6.0)
        head, tail = (None, stream, p(c2w), None, 1, k, VIEWS, VIEW, VIEW, N), (near, far, p(o), p(d), p(t))
        if name == "plain":
            return lib.knerf_generate_rays(*head, FOCAL * 2, *tail)
        if name == "ext_ndc":
            return lib.knerf_generate_rays_ext(*head, FOCAL * 2, *tail, C.byref(ndc))
        cam = view_cams[name]
        cs = cam.c_struct()
        return lib.knerf_generate_rays_cam(*head, p(tables[id(cam)]), 1, C.byref(cs), *tail, C.byref(ndc) if name.endswith("ndc") else None)

    names = ["plain", "cam_plain", "cam_intrinsics", "cam_opencv", "cam_fisheye", "ext_ndc", "cam_opencv_ndc"]
    variants = [(f"{kind}_{name}", fn, name) for kind, fn in (("ray_batch", batch), ("views", views)) for name in names]
    spent = {label: [] for label, _, _ in variants}
    for label, fn, name in variants:                          # warm-up: code objects loaded, every shape launched once
        assert fn(name, 0) == 0, (label, lib.knerf_last_error(None))
    torch.cuda.synchronize()
    for _ in range(repeats):
        for label, fn, name in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(n_launches):
                fn(name, k)
            e1.record(); torch.cuda.synchronize()
            spent[label].append(e0.elapsed_time(e1) / n_launches * 1e3)
    return {label: {"us_per_launch": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2),
                    "rounds": [round(x, 2) for x in v]} for label, v in spent.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camera_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("camera_bench needs the GPU: there is nothing to time without one")
    out = {"tool": "camera_bench", "device": torch.cuda.get_device_name(0),
           "ray_batch": {"rays": RAYS, "samples": N, "views": V, "image": [H, W]}, "views": {"views": VIEWS, "image": [VIEW, VIEW], "samples": N},
           "launches_timed": [args.launches, args.repeats], "newton_steps": 8}
    out["launch_us"] = time_launches(args.launches, args.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
