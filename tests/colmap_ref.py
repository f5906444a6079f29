"""A small writer of COLMAP sparse models (cameras / images / points3D as .bin and .txt) and of binary PPM / PGM files, for the dataset
reader's tests. Written from the format definitions (COLMAP's documentation, "Output Format"): every field is packed explicitly with
struct, little-endian, no padding.
  cameras.bin   u64 count; per camera: u32 camera_id, i32 model_id, u64 width, u64 height, f64 params[model]
  images.bin    u64 count; per image: u32 image_id, f64 qvec[4] (w, x, y, z), f64 tvec[3], u32 camera_id, name + NUL, u64 n_points2D,
                per 2D point: f64 x, f64 y, u64 point3D_id
  points3D.bin  u64 count; per point: u64 point3D_id, f64 xyz[3], u8 rgb[3], f64 error, u64 track_length, per element: u32 image_id,
                u32 point2D_idx
  the .txt files carry the same fields, one record per line ('#' comments; images.txt: a second line of 2D points per image)."""
import os
import struct
import numpy as np

MODEL_IDS = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1, "SIMPLE_RADIAL": 2, "RADIAL": 3, "OPENCV": 4}
MODEL_PARAMS = {"SIMPLE_PINHOLE": 3, "PINHOLE": 4, "SIMPLE_RADIAL": 4, "RADIAL": 5, "OPENCV": 8}


def camera_record(cam):
    """cam = dict(id, model, width, height, params)"""
    assert len(cam["params"]) == MODEL_PARAMS[cam["model"]]
    return (struct.pack("<I", cam["id"]) + struct.pack("<i", MODEL_IDS[cam["model"]]) + struct.pack("<Q", cam["width"]) +
            struct.pack("<Q", cam["height"]) + b"".join(struct.pack("<d", float(p)) for p in cam["params"]))


def image_record(im):
    """im = dict(id, q (w, x, y, z), t, camera_id, name, points2d = [(x, y, point3D_id)])"""
    b = struct.pack("<I", im["id"])
    b += b"".join(struct.pack("<d", float(v)) for v in im["q"])
    b += b"".join(struct.pack("<d", float(v)) for v in im["t"])
    b += struct.pack("<I", im["camera_id"]) + im["name"].encode() + b"\0"
    pts = im.get("points2d", [])
    b += struct.pack("<Q", len(pts))
    for x, y, pid in pts:
        b += struct.pack("<d", x) + struct.pack("<d", y) + struct.pack("<Q", pid & 0xFFFFFFFFFFFFFFFF)
    return b


def point_record(pt):
    """pt = dict(id, xyz, rgb, error, track = [(image_id, point2D_idx)])"""
    b = struct.pack("<Q", pt["id"]) + b"".join(struct.pack("<d", float(v)) for v in pt["xyz"])
    b += b"".join(struct.pack("<B", int(v)) for v in pt["rgb"]) + struct.pack("<d", float(pt.get("error", 0.5)))
    tr = pt.get("track", [])
    b += struct.pack("<Q", len(tr))
    for iid, idx in tr:
        b += struct.pack("<I", iid) + struct.pack("<I", idx)
    return b


def sparse_bin(cameras, images, points):
    """-> {file name: bytes}"""
    return {"cameras.bin": struct.pack("<Q", len(cameras)) + b"".join(camera_record(c) for c in cameras),
            "images.bin": struct.pack("<Q", len(images)) + b"".join(image_record(i) for i in images),
            "points3D.bin": struct.pack("<Q", len(points)) + b"".join(point_record(p) for p in points)}


def sparse_txt(cameras, images, points):
    cam = "# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n"
    for c in cameras:
        cam += " ".join([str(c["id"]), c["model"], str(c["width"]), str(c["height"])] + [repr(float(p)) for p in c["params"]]) + "\n"
    img = "# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n#   POINTS2D[] as (X, Y, POINT3D_ID)\n"
    for i in images:
        img += " ".join([str(i["id"])] + [repr(float(v)) for v in i["q"]] + [repr(float(v)) for v in i["t"]] + [str(i["camera_id"]), i["name"]]) + "\n"
        img += " ".join(f"{x!r} {y!r} {pid}" for x, y, pid in i.get("points2d", [])) + "\n"
    pts = "# 3D point list with one line of data per point:\n#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n"
    for p in points:
        pts += " ".join([str(p["id"])] + [repr(float(v)) for v in p["xyz"]] + [str(int(v)) for v in p["rgb"]] + [repr(float(p.get("error", 0.5)))] +
                        [f"{a} {b}" for a, b in p.get("track", [])]) + "\n"
    return {"cameras.txt": cam.encode(), "images.txt": img.encode(), "points3D.txt": pts.encode()}


def write_ppm(path, rgb):
    """rgb uint8 [H][W][3]"""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w, _ = rgb.shape
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h) + rgb.tobytes())


def write_pgm(path, gray):
    gray = np.ascontiguousarray(gray, np.uint8)
    h, w = gray.shape
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (w, h) + gray.tobytes())


def write_dataset(root, cameras, images, points, pixels=None, binary=True, sparse_sub="sparse/0", masks=None):
    """pixels: {image name: uint8 [H][W][3]} written as images/<stem>.ppm; masks: {image name: uint8 [H][W]} as masks/<stem>.pgm"""
    sp = os.path.join(root, sparse_sub)
    os.makedirs(sp, exist_ok=True)
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    for name, data in (sparse_bin if binary else sparse_txt)(cameras, images, points).items():
        with open(os.path.join(sp, name), "wb") as f:
            f.write(data)
    for name, px in (pixels or {}).items():
        write_ppm(os.path.join(root, "images", os.path.splitext(name)[0] + ".ppm"), px)
    if masks:
        os.makedirs(os.path.join(root, "masks"), exist_ok=True)
        for name, m in masks.items():
            write_pgm(os.path.join(root, "masks", os.path.splitext(name)[0] + ".pgm"), m)


def rotmat_to_qvec(R):
    """row-major world -> camera rotation -> (w, x, y, z), w >= 0 (the largest-component branch form)"""
    R = np.asarray(R, np.float64)
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif R[1, 1] > R[2, 2]:
        s = np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        s = np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    q = np.array(q)
    return -q if q[0] < 0 else q


def qvec_to_rotmat(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]])
