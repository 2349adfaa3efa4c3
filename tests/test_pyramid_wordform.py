"""k_pyramid's word-aligned fixed point on the GPU: every pixel of every level
against the oracle, on frames that reach the arithmetic's extremes
(D = 255 * 2048 on saturated frames, 0 / 255 neighbours on checkerboards) and
on a width that gives odd pitches: all four byte alignments of the 8-byte
source window and the unaligned staging path."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(160, 120), (203, 131)]
FRAMES = ["white", "black", "checker1", "checker2", "random"]
PYRAMIDS = [(8, 1.2), (4, 1.5)]  # (levels, scale)


def _frame(kind, w, h):
    if kind == "white":
        return np.full((h, w), 255, np.uint8)
    if kind == "black":
        return np.zeros((h, w), np.uint8)
    if kind.startswith("checker"):
        p = int(kind[-1])
        y, x = np.mgrid[0:h, 0:w]
        return ((((x // p) + (y // p)) & 1) * 255).astype(np.uint8)
    return np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w), dtype=np.uint8)


@pytest.mark.parametrize("L,sf", PYRAMIDS)
@pytest.mark.parametrize("kind", FRAMES)
@pytest.mark.parametrize("w,h", SIZES)
def test_levels_match_oracle(gpu, oracle, w, h, kind, L, sf):
    img = _frame(kind, w, h)
    ref = oracle.Extractor(200, sf, L, 20, 7, cell_guard="empty")
    ref.extract(img)
    ex = gpu.Extractor(200, sf, L, 20, 7, cell_guard="empty")
    ex.extract(img)
    for l in range(L):
        a, b = ex.level(l), ref.level(l)
        assert a.shape == b.shape, "level %d shape" % l
        assert np.array_equal(a, b), "level %d: %d pixels differ" % (l, int((a != b).sum()))
    if kind == "white":  # INTER_LINEAR of a constant: the saturated extreme survives every level
        assert all(int(ref.level(l).min()) == 255 for l in range(L))
