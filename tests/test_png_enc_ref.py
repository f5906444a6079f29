"""tests/png_enc_ref.py, the restatement dvs_png_encode_views is held against (tests/test_gpu_png_encode.py), checked on the CPU against
what is independent of it: png_ref.unfilter (the decoder's restatement) gives the raw bytes back for all three kinds; over the shared
test images every filter 0..4 is chosen at least once; a row of zeros gets filter 0; the sample rule on the k + 0.5 ties, NaN, +-inf,
values below 0 and above M / scale; and the GRAY8 rule at scale 255 is jpeg_enc_ref's float -> byte step."""
import numpy as np
import pytest
import jpeg_enc_ref as JE
import png_enc_ref as PE
import png_ref

SHAPES = [(1, 1), (3, 2), (17, 5), (64, 48), (257, 9), (1030, 3), (40, 1)]
SCALES = [255.0, 1000.0, 65535.0]


def pictures(W, H):
    return [PE.image(W, H, W + H)] + PE.specials(W, H) + [PE.smooth(W, H)]


@pytest.mark.parametrize("kind", PE.KINDS, ids=["rgb8", "gray8", "gray16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_decoder_restatement_gives_the_raw_bytes_back(shape, kind):
    W, H = shape
    ctype, depth = PE.PNG_TYPE[kind]
    for img in pictures(W, H):
        for scale in SCALES:
            x = PE.plane_of(img, kind)
            stream, choice, _ = PE.encode(x, scale, kind)
            raw, _ = PE.raw_rows(x, scale, kind)
            assert stream.size == H * (1 + W * PE.BPP[kind]) and raw.shape == (H, W * PE.BPP[kind])
            assert np.array_equal(stream.reshape(H, -1)[:, 0], choice) and choice.max() <= 4
            assert np.array_equal(png_ref.unfilter(stream, W, H, depth, ctype), raw)


def test_every_filter_is_chosen_over_the_test_images():
    seen = {kind: set() for kind in PE.KINDS}
    for W, H in SHAPES:
        for img in pictures(W, H):
            for kind in PE.KINDS:
                for scale in SCALES:
                    seen[kind] |= set(PE.encode(PE.plane_of(img, kind), scale, kind)[1].tolist())
    print({k: sorted(v) for k, v in seen.items()})
    assert all(v == {0, 1, 2, 3, 4} for v in seen.values()), seen          # by every kind


def test_a_row_of_zeros_gets_filter_0_and_ties_go_to_the_smallest():
    for kind in PE.KINDS:
        z = np.zeros((3, 4, 9), np.float32)
        stream, choice, nsat = PE.encode(PE.plane_of(z, kind), 255.0, kind)
        assert choice.tolist() == [0, 0, 0, 0] and not stream.any() and nsat == 0
        # a constant picture: the first row ties None with Up (no row above) and takes None or Sub by cost; every later row is zeros under Up
        c = np.full((3, 4, 9), 0.5, np.float32)
        stream, choice, _ = PE.encode(PE.plane_of(c, kind), 255.0, kind)
        assert choice[1:].tolist() == [2, 2, 2] and not stream.reshape(4, -1)[1:, 1:].any()
        cost0 = PE.costs(PE.filtered_rows(PE.raw_rows(PE.plane_of(c, kind), 255.0, kind)[0], PE.BPP[kind]))[0]
        assert choice[0] == int(np.flatnonzero(cost0 == cost0.min())[0]) and cost0[0] == cost0[2]


def test_the_sample_rule_on_ties_and_special_values():
    for kind, scale in ((PE.GRAY8, 255.0), (PE.GRAY16, 1000.0), (PE.GRAY16, 65535.0), (PE.RGB8, 255.0)):
        M = PE.MAX_SAMPLE[kind]
        k = np.arange(0, 64, dtype=np.float64)
        x = ((k + 0.5) / scale).astype(np.float32)
        prod = x * np.float32(scale)
        ties = prod - np.floor(prod) == 0.5
        assert ties.sum() >= 8                                              # real ties among them
        s, sat = PE.quantise(x, scale, kind)
        f = np.floor(prod.astype(np.float64))
        want = np.where(ties, f + f % 2, np.floor(prod.astype(np.float64) + 0.5))      # a tie goes to the even neighbour, the rest to the nearest
        assert np.array_equal(s, want.astype(np.int64)) and not sat.any()
        big = np.float32(np.nextafter(np.float32((M + 0.5) / scale), np.float32(np.inf)))
        v = np.array([np.nan, np.inf, -np.inf, -0.0, -3.5, 0.0, M / scale, big * 2, 1e30, -1e30, 1e-30], np.float32)
        s, sat = PE.quantise(v, scale, kind)
        assert s[:6].tolist() == [0, M, 0, 0, 0, 0] and s[7:].tolist() == [M, M, 0, 0]
        assert sat.tolist() == [False, True, False, False, False, False, bool(np.rint(v[6] * np.float32(scale)) > M), True, True, False, False]
        assert s[6] in (M - 1, M)
    # high byte first, R G B interleaved, and the count of saturated samples
    raw, nsat = PE.raw_rows(np.array([[0.258, 70.0]], np.float32), 1000.0, PE.GRAY16)
    assert raw.tolist() == [[1, 2, 255, 255]] and nsat == 1
    rgb = np.array([[[0.0, 1.0]], [[0.2, 2.0]], [[1.0, np.nan]]], np.float32)
    raw, nsat = PE.raw_rows(rgb, 255.0, PE.RGB8)
    assert raw.tolist() == [[0, 51, 255, 255, 255, 0]] and nsat == 1


def test_gray8_at_255_is_the_jpeg_encoder_float_to_byte_step():
    r = np.random.default_rng(3)
    x = r.uniform(-0.2, 1.2, (3, 40, 24)).astype(np.float32)
    x[0, 0, :6] = [np.nan, np.inf, -np.inf, -0.0, 7.25, 1.0]
    x[1] = ((r.integers(0, 255, (40, 24)) + 0.5) / 255.0).astype(np.float32)
    for p in range(3):
        assert np.array_equal(PE.raw_rows(x[p], 255.0, PE.GRAY8)[0], JE.to_bytes(x)[p])
    assert np.array_equal(PE.raw_rows(x, 255.0, PE.RGB8)[0].reshape(40, 24, 3).transpose(2, 0, 1), JE.to_bytes(x))
