"""Writes tests/golden/jpeg_enc_expected.npz, the recorded PIL side of tests/test_jpeg_write_format.py. Run once by hand (it imports PIL;
no test does):  python tests/golden/make_jpeg_enc_fixtures.py
  quant/<Q>/luma, quant/<Q>/chroma   uint16[64], natural order: the tables PIL writes at quality Q in 1, 25, 50, 75, 90, 95, 100, read
                                     back from the DQT segments of its file by tests/jpeg_ref.py
  noise_40x24                        uint8 [3][24][40]: the random-noise image of the fidelity check (seed 2024)
  pil_psnr/<image>/<Q>/<420|444>     float64: PSNR(PIL decode(PIL encode(image, Q, sampling)), image), Q in 50, 90, 100; the images are
                                     the pixels jpeg_ref.decode gives for every accepted fixture of tests/golden/jpeg/, and the noise image"""
import glob
import io
import os
import sys
import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_ref as J            # noqa: E402
import jpeg_enc_ref as E        # noqa: E402

QUALITIES = (1, 25, 50, 75, 90, 95, 100)
FIDELITY_Q = (50, 90, 100)


def images():
    out = {}
    for f in sorted(glob.glob(os.path.join(HERE, "jpeg", "*.jpg"))):
        name = os.path.basename(f)[:-4]
        if name in ("progressive", "adobe_rgb"):
            continue
        out[name] = J.decode(open(f, "rb").read())
    out["noise_40x24"] = np.random.default_rng(2024).integers(0, 256, (3, 24, 40)).astype(np.uint8)
    return out


def pil_bytes(img, quality, sampling):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img.transpose(1, 2, 0)), "RGB").save(buf, "JPEG", quality=quality, subsampling=0 if sampling == "444" else 2)
    return buf.getvalue()


def main():
    rec = {}
    flat = np.full((3, 16, 16), 128, np.uint8)
    for q in QUALITIES:
        f = J.decode_coefficients(pil_bytes(flat, q, "420"))
        assert np.array_equal(f.quant[1], f.quant[2])
        rec[f"quant/{q}/luma"], rec[f"quant/{q}/chroma"] = f.quant[0], f.quant[1]
    imgs = images()
    rec["noise_40x24"] = imgs["noise_40x24"]
    for name, img in imgs.items():
        for q in FIDELITY_Q:
            for s in ("420", "444"):
                back = np.asarray(Image.open(io.BytesIO(pil_bytes(img, q, s))).convert("RGB")).transpose(2, 0, 1)
                rec[f"pil_psnr/{name}/{q}/{s}"] = np.float64(E.psnr(back, img))
    np.savez_compressed(os.path.join(HERE, "jpeg_enc_expected.npz"), **rec)
    print(len(rec), "records")


if __name__ == "__main__":
    main()
