"""Plain numpy restatement of the preview images of the inference drivers, on a [z, y, x] float32 array `dim_output`:
the 8-bit quantisation, the stacked axis sums, the slice loop with its gate and its file names, a float64 version of the
sums with the bound a float32 sum has to meet, and the data the GPU tests use."""
import numpy as np

GATE = 0.0001
DUMP_FRAME = 110
U = 2.0 ** -24                      # unit roundoff of float32


def save_img(img):
    """uint8(clip(img * 255, 0, 255)): a float32 product, truncated"""
    img = np.asarray(img, dtype=np.float32)
    return np.clip(img * np.float32(255.0), 0, 255).astype(np.uint8)


def axis_sums(img):
    img = np.asarray(img, dtype=np.float32)
    return [np.sum(img, axis=k, dtype=np.float32) for k in range(3)]


def save_img_3d(img):
    """the three axis sums stacked along the rows (all three as wide as the last axis), quantised"""
    return save_img(np.concatenate(axis_sums(img), axis=0))


def projection(dim_output, divisor=80.0):
    return save_img_3d(np.asarray(dim_output, dtype=np.float32) / np.float32(divisor))


def slice_planes(dim_output, i):
    """the three images of index i: xy = plane i of axis 0; yz = plane i of axis 2, transposed; xz = plane i of axis 1"""
    d = np.asarray(dim_output, dtype=np.float32)
    return {"slice_xy": save_img(d[i]), "slice_yz": save_img(d.transpose(2, 1, 0)[i]), "slice_xz": save_img(d.transpose(1, 0, 2)[i])}


def gate(dim_output, i):
    return bool(np.average(np.asarray(dim_output, dtype=np.float32)[i]) > GATE)


def slice_files(dim_output, frame_no, tile_size_high):
    """{file name: image} of the slice loop: the two mid planes named <kind>_<i>_<frame>, and for frame 110 the planes
    0 .. tile_size_high - 1 named <kind>_<frame>_<i>; an index is written when the mean of its xy plane exceeds the gate"""
    size = np.shape(dim_output)[0]
    files = {}
    for i in range(size // 2 - 1, size // 2 + 1):
        if gate(dim_output, i):
            for kind, img in slice_planes(dim_output, i).items():
                files["%s_%04d_%04d.png" % (kind, i, frame_no)] = img
    if frame_no == DUMP_FRAME:
        for i in range(0, tile_size_high):
            if gate(dim_output, i):
                for kind, img in slice_planes(dim_output, i).items():
                    files["%s_%04d_%04d.png" % (kind, frame_no, i)] = img
    return files


def source_name(frame_no, tag=None):
    return "source_%04d.png" % frame_no if tag is None else "source_%s_%04d.png" % (tag, frame_no)


def frame_files(pass_outputs, final, frame_no, tile_size_high):
    """every file of one frame of the multi-network driver: pass_outputs = [(tag, dim_output at that pass)], final = the
    dim_output of the slice loop"""
    files = {source_name(frame_no, tag): projection(d) for tag, d in pass_outputs}
    files.update(slice_files(final, frame_no, tile_size_high))
    return files


class NumpyImages(object):
    """what mpgan_amd.preview offers a PreviewSink, on numpy arrays"""

    @staticmethod
    def projection_image(vol, perm=(0, 1, 2), divisor=80.0):
        return projection(np.asarray(vol).transpose(perm), divisor)

    @staticmethod
    def slice_images(vol, perm, indices):
        d = np.asarray(vol).transpose(perm)
        out = {"slice_xy": [], "slice_yz": [], "slice_xz": []}
        for i in indices:
            if gate(d, i):
                for kind, img in slice_planes(d, i).items():
                    out[kind].append((i, img))
        return out


# ------------------------------------------------------------------------------------------------ float64 and bounds
def sums64(vol, divisor=80.0):
    """per axis (r, bound): r the float64 sum of v / divisor, bound = (n + 1) 2^-24 sum |v / divisor| -- what a float32 sum
    of n correctly rounded quotients can be off by, in any order: n - 1 additions and one division per term"""
    q = np.asarray(vol, dtype=np.float64) / float(divisor)
    return [(q.sum(axis=k), (q.shape[k] + 1) * U * np.abs(q).sum(axis=k)) for k in range(3)]


def stacked_bounds(dim_output, divisor=80.0):
    """(lowest, highest) grey level of every pixel of the stacked image whose float lies within the bound"""
    s = sums64(dim_output, divisor)
    r = np.concatenate([x for x, _ in s], axis=0)
    b = np.concatenate([x for _, x in s], axis=0)
    return save_img64(r - b), save_img64(r + b)


def save_img64(img):
    """the grey level of a real number: the float32 nearest to it, quantised as save_img does"""
    return save_img(np.asarray(img, dtype=np.float64).astype(np.float32))


def mean_bound(plane):
    """float64 mean of a plane and n 2^-24 mean|v|: the error of a float32 sum in any order plus the division"""
    p = np.asarray(plane, dtype=np.float64)
    return p.mean(), p.size * U * np.abs(p).mean()


# ------------------------------------------------------------------------------------------------ data of the GPU tests
EXACT_SHAPES = [(1, 1, 1), (3, 5, 5), (5, 7, 7), (6, 10, 7), (16, 64, 64), (64, 64, 64), (130, 96, 96)]
GENERAL_SHAPES = [(5, 7, 7), (130, 96, 96)]


def exact_volume(shape, seed=0):
    """v = 5 k 2^-6, k integer in [0, 12]: v / 80 = k 2^-10 exactly, and a sum of up to 512 of them is an integer below
    2^13 times 2^-10 -- exact in float32 in any order"""
    k = np.random.default_rng(seed).integers(0, 13, size=shape)
    return (5.0 * k * 2.0 ** -6).astype(np.float32)


def general_volume(shape, seed=1):
    return (np.random.default_rng(seed).random(shape) ** 3).astype(np.float32)


def gated_volume(shape, seed=2):
    """xy planes (axis 0) that are all zero (every third one, from plane 1) or have a mean of at least 1e-3"""
    v = general_volume(shape, seed) + np.float32(0.01)
    v[1::3] = 0
    return v


def exactness_holds(vol, divisor=80.0):
    """the quotients are multiples of 2^-10 and no axis sum reaches 2^24 of them"""
    q = np.asarray(vol, dtype=np.float64) / divisor * 2.0 ** 10
    return bool(np.all(q == np.round(q)) and max(q.sum(axis=k).max() for k in range(3)) < 2 ** 24 and
                np.array_equal((np.asarray(vol, np.float32) / np.float32(divisor)).astype(np.float64) * 2.0 ** 10, q))


def gate_margin(dim_output):
    """smallest distance of an xy plane mean from the gate"""
    d = np.asarray(dim_output, dtype=np.float64)
    return float(np.min(np.abs(d.mean(axis=(1, 2)) - GATE)))
