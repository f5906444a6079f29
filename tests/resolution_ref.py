"""numpy restatement of the coarse-to-fine schedule (resolutionSchedule / numDownscales) — TEST INFRASTRUCTURE, not product code:
the level of a step, the box downsample of dvs_downsample_views in its defined operation order (so that it can be compared bit for
bit), and the level camera of dvs_camera_downscale. Shared by tests/test_resolution_abi.py, test_gpu_downsample.py and
test_resolution_schedule.py."""
import numpy as np


def level_of_step(step, every, levels):
    """level k of the step that follows `step` completed ones: max(K - step // S, 0); 0 when the schedule is off (S <= 0)"""
    return max(int(levels) - int(step) // int(every), 0) if every > 0 else 0


def clamp_levels(levels, W, H):
    """K as the trainer clamps it once at load: at most 3 (factor 8), and the largest value with min(W, H) >> K >= 16"""
    k = max(0, min(int(levels), 3))
    while k > 0 and (min(W, H) >> k) < 16:
        k -= 1
    return k


def downsample_np(src, factor):
    """[planes, H, W] uint8 or float32 -> float32 [planes, H // f, W // f], the plain mean of each f x f block in the kernel's order:
    uint8   (float32(S) * float32(1/255)) * float32(1/(f f)), S the exact integer sum of the block
    float32 the block's values added in float32 in row-major order, starting from the first, then * float32(1/(f f))
    The W - (W // f) f rightmost columns and the matching bottom rows are not used."""
    src = np.asarray(src)
    f = int(factor)
    planes, H, W = src.shape
    Hd, Wd = H // f, W // f
    inv = np.float32(1.0) / np.float32(f * f)
    blocks = src[:, :Hd * f, :Wd * f].reshape(planes, Hd, f, Wd, f)
    if src.dtype == np.uint8:
        S = blocks.astype(np.uint32).sum(axis=(2, 4))
        return ((S.astype(np.float32) * (np.float32(1.0) / np.float32(255.0))) * inv).astype(np.float32)
    assert src.dtype == np.float32, src.dtype
    acc = None
    for r in range(f):
        for c in range(f):
            v = blocks[:, :, r, :, c]
            acc = v.copy() if acc is None else (acc + v).astype(np.float32)
    return (acc * inv).astype(np.float32)


def camera_downscale_np(cam, factor):
    """the level camera as a dict of every dvs_camera field (float32 arrays / ints): view, campos, bg unchanged; width, height floor
    divided; focal / d; with s = size / (d level size) in float64, proj row r' = s proj row r + (s - 1) proj row 3 for r = 0 (x) and
    1 (y), tan_fov / s — and untouched (bit for bit) where s == 1"""
    d = int(factor)
    W, H = int(cam.width), int(cam.height)
    Wd, Hd = W // d, H // d
    proj = np.array(list(cam.proj), np.float32)
    tan = [np.float32(cam.tan_fovx), np.float32(cam.tan_fovy)]
    if d > 1:
        for r, s in enumerate((np.float64(W) / (np.float64(d) * Wd), np.float64(H) / (np.float64(d) * Hd))):
            if s == 1.0:
                continue
            p64 = proj.astype(np.float64)
            for k in range(4):
                proj[k * 4 + r] = np.float32(s * p64[k * 4 + r] + (s - 1.0) * p64[k * 4 + 3])
            tan[r] = np.float32(np.float64(tan[r]) / s)
    return dict(view=np.array(list(cam.view), np.float32), proj=proj, tan_fovx=tan[0], tan_fovy=tan[1],
                focal_x=np.float32(cam.focal_x) / np.float32(d), focal_y=np.float32(cam.focal_y) / np.float32(d),
                campos=np.array(list(cam.campos), np.float32), width=Wd, height=Hd, bg=np.array(list(cam.bg), np.float32))


def camera_fields(cam):
    """every field of a ctypes dvs_camera in the form camera_downscale_np returns"""
    return dict(view=np.array(list(cam.view), np.float32), proj=np.array(list(cam.proj), np.float32), tan_fovx=np.float32(cam.tan_fovx),
                tan_fovy=np.float32(cam.tan_fovy), focal_x=np.float32(cam.focal_x), focal_y=np.float32(cam.focal_y),
                campos=np.array(list(cam.campos), np.float32), width=int(cam.width), height=int(cam.height), bg=np.array(list(cam.bg), np.float32))


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return np.array_equal(a, b)
