"""Host side of the held-out evaluation: ABI prototypes, the float64 restatement of mpg_logit_stats, the drivers'
test / print / image schedule and the PNG writer.  No GPU."""
import math

import numpy as np

import mpgan_amd  # noqa: F401
from mpgan_amd import _lib, heldout

import heldout_ref as HR


def test_abi_has_the_evaluation_entries():
    lib = _lib.load()
    for name in ("mpg_logit_stats", "mpg_bn_infer_act", "mpg_tiles_to_gray8"):
        assert name in _lib.PROTOTYPES
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.PROTOTYPES[name][1] and fn.restype is _lib.PROTOTYPES[name][0]
    assert len(_lib.PROTOTYPES["mpg_logit_stats"][1]) == 4
    assert len(_lib.PROTOTYPES["mpg_bn_infer_act"][1]) == 15
    assert len(_lib.PROTOTYPES["mpg_tiles_to_gray8"][1]) == 10


def test_logit_stats_restatement_by_hand():
    l = [-2.0, -0.5, 0.0, 1.0, 3.0]
    sig = [1.0 / (1.0 + math.exp(-v)) for v in l]
    want = [sum(l) / 5, sum(sig) / 5,
            sum(-math.log(s) for s in sig) / 5,                 # cross entropy against label 1
            sum(-math.log(1.0 - s) for s in sig) / 5,           # against label 0
            sum((v - 1.0) ** 2 for v in l) / 5, sum(v * v for v in l) / 5]
    got = HR.logit_stats(np.array(l))
    assert np.allclose(got, want, rtol=1e-13, atol=0)
    # the stable form does not overflow where exp(l) would
    big = HR.logit_stats(np.array([-800.0, 800.0]))
    assert np.all(np.isfinite(big)) and abs(big[1] - 0.5) < 1e-15 and abs(big[2] - 400.0) < 1e-12


def test_schedule_matches_the_reference_conditions():
    for total, ti, oi, img in ((12, 2, 2, 1), (12, 3, 4, 1), (10, 100000, 5, -1), (7, 1, 3, 0)):
        for it in range(total):
            want = ((it + 1) % ti == 0, (it + 1) % oi == 0, (it + 1) % oi == 0 and img > -1)
            assert heldout.schedule(it, ti, oi, img) == want, (total, ti, oi, img, it)
    # no test frames: the test section is skipped, reports and images stay
    assert heldout.schedule(1, 2, 2, 1, have_test_data=False) == (False, True, True)
    assert heldout.frame_index(1002, 1000, 120, 3) == 243


def test_report_has_the_reference_fields_in_order():
    log = heldout.HeldOutLog()
    log.add_train("avgCost_disc", 3.0)
    log.add_train("avgCost_gen", 1.0)
    log.sums["avgTestCost_disc_real"], log.sums["avgTestCost_disc_gen"], log.tests = 0.5, 0.25, 1
    text = log.report(1, 10, 2, 1, 1, blend=2.5)
    line = [ln for ln in text.split("\n") if ln.startswith("\tdisc:")][0]
    assert line == ("\tdisc: loss: train_loss=1.500000 - test-real=0.500000 - test-generated=0.250000, "
                    "out: train=0.000000 - test=0.000000")
    assert "\tT D : loss[ -train (total=" in text and "\t gen: loss: train=0.500000 - L1(*k)=" in text
    assert "\t blending percentage: 2.500000" in text
    assert log.tests == 0 and log.sums["avgCost_disc"] == 0.0


def test_png_writer_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (37, 53), dtype=np.uint8)
    img[0, :3] = (0, 255, 128)
    data = heldout.encode_gray_png(img)
    assert np.array_equal(heldout.decode_gray_png(data), img)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        path = tmp_path / "a.png"
        path.write_bytes(data)
        with Image.open(str(path)) as im:
            assert im.mode == "L" and np.array_equal(np.asarray(im), img)
    heldout.write_gray_png(str(tmp_path / "b.png"), img)
    raw = (tmp_path / "b.png").read_bytes()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
