"""Host side of the held-out evaluation of the training drivers: when the loop tests / prints / writes an image
(multipassGAN-4x.py:1411,1519,1581; -8x.py:2095,2199,2263), the running averages of the test section and the
reference's report lines, and the 8-bit PNG of the test image."""
import struct
import zlib

import numpy as np


def schedule(it, test_interval, output_interval, gen_test_img=-1, have_test_data=True):
    """-> (test now, print now, image now) for the 0-based iteration `it`, the conditions of the reference loop:
    `(it + 1) % testInterval == 0`, `(it + 1) % outputInterval == 0`, and an image with every report when
    genTestImg > -1.  Without test frames the test section is skipped."""
    test_now = bool(have_test_data) and test_interval > 0 and (it + 1) % test_interval == 0
    print_now = output_interval > 0 and (it + 1) % output_interval == 0
    return test_now, print_now, print_now and gen_test_img > -1


def frame_index(sim_no, from_sim, frame_max, frame_no=0):
    """index of generateTestImage's frame in the tile creator's data (4x.py:1055)"""
    return (sim_no - from_sim) * frame_max + frame_no


# accumulator name of the reference -> key of Trainer*.evaluate
_TEST_FIELDS = (
    ("avgOut_disc", "out_disc_train"), ("avgOut_gen", "out_gen_train"),
    ("avgTestCost_disc_real", "d_loss_y"), ("avgTestCost_disc_gen", "d_loss_g"), ("avgTestCost_gen", "g_loss_d"),
    ("avgTestOut_disc_real", "out_disc_test"), ("avgTestOut_disc_gen", "out_gen_test"),
    ("avgOut_disc_t", "t_out_disc_train"), ("avgOut_gen_t", "t_out_gen_train"),
    ("avgTestCost_disc_real_t", "t_loss_y"), ("avgTestOut_disc_real_t", "t_out_disc_test"),
    ("avgTestCost_disc_gen_t", "t_loss_g"), ("avgTestOut_disc_gen_t", "t_out_gen_test"),
    ("avgTestCost_gen_t", "g_loss_t"), ("avgTestCost_gen_t_l", "tl_gen_loss"),
)
_TRAIN_FIELDS = ("avgCost_disc", "avgCost_gen", "avgL1Cost_gen", "avgTemCost_disc", "avgTemCost_gen", "avgTemCost_gen_l")


class HeldOutLog(object):
    """the running sums between two reports: training costs added per update, test quantities per evaluate() call"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.tests = 0
        self.sums = {name: 0.0 for name, _ in _TEST_FIELDS}
        self.sums.update({name: 0.0 for name in _TRAIN_FIELDS})
        self._pending = {}          # name -> device sum of the scalars added since the last report

    def add_train(self, name, value):
        """value: a device scalar (summed on the device, transferred with the report: no synchronisation per update) or a
        number"""
        if hasattr(value, "detach"):
            v = value.detach().reshape(()).double()
            self._pending[name] = v if name not in self._pending else self._pending[name] + v
        else:
            self.sums[name] += float(value)

    def _flush(self):
        if self._pending:
            import torch
            names = sorted(self._pending)
            for name, v in zip(names, torch.stack([self._pending[n] for n in names]).cpu().numpy()):
                self.sums[name] += float(v)
            self._pending = {}

    def add_test(self, result):
        """result: the dict of Trainer*.evaluate (device scalars: one transfer for all of them)"""
        import torch
        keys = [(name, key) for name, key in _TEST_FIELDS if key in result]
        vals = torch.stack([result[key].detach().reshape(()) for _, key in keys]).cpu().numpy()
        for (name, _), v in zip(keys, vals):
            self.sums[name] += float(v)
        self.tests += 1

    def report(self, it, total, output_interval, disc_runs, gen_runs, k=1.0, kt=0.0, kt_l=0.0, blend=None):
        # 'Epoch' heads the report in both reference loops (4x.py:1551, and 8x.py:2231 although it counts iterations)
        """the report lines of the reference (4x.py:1551-1573, 8x.py:2231-2255), its wording and field order; -> the text"""
        self._flush()
        s = dict(self.sums)
        for name in ("avgCost_disc", "avgTemCost_disc"):
            s[name] /= float(output_interval * disc_runs)
        for name in ("avgCost_gen", "avgL1Cost_gen", "avgTemCost_gen", "avgTemCost_gen_l"):
            s[name] /= float(output_interval * gen_runs)
        if self.tests:
            for name, _ in _TEST_FIELDS:
                s[name] /= float(self.tests)
        lines = ['\nEpoch {:05d}/{}, Cost:'.format(it + 1, total),
                 '\tdisc: loss: train_loss={:.6f} - test-real={:.6f} - test-generated={:.6f}, out: train={:.6f} - test={:.6f}'
                 .format(s["avgCost_disc"], s["avgTestCost_disc_real"], s["avgTestCost_disc_gen"], s["avgOut_disc"],
                         s["avgTestOut_disc_real"]),
                 '\tT D : loss[ -train (total={:.6f}), -test (real&1={:.6f}) (generated&0={:.6f})]'
                 .format(s["avgTemCost_disc"], s["avgTestCost_disc_real_t"], s["avgTestCost_disc_gen_t"]),
                 '\t	sigmoidout[ -test (real&1={:.6f}) (generated&0={:.6f})'
                 .format(s["avgTestOut_disc_real_t"], s["avgTestOut_disc_gen_t"]),
                 '\t gen: loss: train={:.6f} - L1(*k)={:.3f} - test={:.6f}, DS out: train={:.6f} - test={:.6f}'
                 .format(s["avgCost_gen"], s["avgL1Cost_gen"] * k, s["avgTestCost_gen"], s["avgOut_gen"],
                         s["avgTestOut_disc_gen"]),
                 '\t gen: loss[ -train (total Temp(*k)={:.6f}) -test (total Temp(*k)={:.6f})], DT out: real={:.6f} - gen={:.6f}'
                 .format(s["avgTemCost_gen"] * kt, s["avgTestCost_gen_t"] * kt, s["avgOut_disc_t"], s["avgOut_gen_t"])]
        if blend is not None:
            lines.append('\t blending percentage: %f' % blend)
        lines.append('\t l2 tempo loss[ -train (total Temp(*k)={:.6f}) -test (total Temp(*k)={:.6f})]'
                     .format(s["avgTemCost_gen_l"] * kt_l, s["avgTestCost_gen_t_l"] * kt_l))
        self.reset()
        return "\n".join(lines)


# ------------------------------------------------------------------------------------------------ PNG
def encode_gray_png(img):
    """[H, W] uint8 -> the bytes of an 8-bit greyscale PNG (zlib + struct: filter 0 on every row)"""
    img = np.ascontiguousarray(img)
    if img.ndim != 2 or img.dtype != np.uint8:
        raise ValueError("encode_gray_png: expected a [H, W] uint8 array, got %s %s" % (img.shape, img.dtype))
    h, w = img.shape

    def chunk(tag, data):
        body = tag + data
        return struct.pack(">I", len(data)) + body + struct.pack(">I", zlib.crc32(body) & 0xffffffff)

    raw = np.concatenate([np.zeros((h, 1), np.uint8), img], axis=1).tobytes()
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) +
            chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def decode_gray_png(data):
    """inverse of encode_gray_png for its own output (8-bit grey, filter 0, no interlace) -> [H, W] uint8"""
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("not a PNG")
    pos, idat, w = 8, b"", None
    while pos < len(data):
        (n,), tag = struct.unpack(">I", data[pos:pos + 4]), data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            w, h, depth, colour, _, _, interlace = struct.unpack(">IIBBBBB", body)
            if (depth, colour, interlace) != (8, 0, 0):
                raise ValueError("decode_gray_png reads 8-bit greyscale without interlace only")
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, w + 1)
    if rows[:, 0].any():
        raise ValueError("decode_gray_png reads filter type 0 only")
    return rows[:, 1:].copy()


def write_gray_png(path, img):
    """Pillow when it imports, as tilecreator_t.savePngsGrayscale uses it; otherwise the writer above"""
    try:
        from PIL import Image
    except ImportError:
        with open(path, "wb") as f:
            f.write(encode_gray_png(img))
        return
    Image.fromarray(np.ascontiguousarray(img, dtype=np.uint8)).save(path)

