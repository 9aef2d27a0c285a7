"""Float64 restatement of what mpg_slice_zoom_means / mpg_slice_zoom_gather (csrc/mpgan_loader.hip) compute, and the
synthetic simulation directory the loader tests share.  test_loader_device_host.py proves on the CPU what is claimed
here (agreement with scipy.ndimage.zoom); test_loader_device_gpu.py holds the kernels against it.

The virtual array: V = zoom(transpose(src, perm + (3,)), factors), order 1.  Along an axis of n source and `big` output
points scipy reads output index o at the coordinate o * ((n - 1) / (big - 1)) -- the ratio is formed first, as a Python
float, the product in C -- or o * 1.0 where big == 1, and with its default mode 'constant' writes 0 where that
coordinate leaves [0, n - 1] (the last index can, by one rounding).  The interpolation is separable."""
import os

import numpy as np

SLICE_AXES = {0: (None, None), 1: ((1, 0, 2, 3), (2, 3)), 2: ((2, 1, 0, 3), (1, 3))}      # fluiddataloader._View


def out_size(n, factor):
    return int(round(n * factor))


def axis_table(n, big):
    """-> lower index, upper index, upper weight (float64), zero flag, for the `big` outputs of an axis of n points"""
    ratio = float(n - 1) / float(big - 1) if big > 1 else 1.0
    cc = np.arange(big, dtype=np.float64) * ratio
    fl = np.floor(cc)
    i0 = np.clip(fl.astype(np.int64), 0, n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    return i0, i1, cc - fl, (cc < 0) | (cc > n - 1)


def zoom_ref(a, out3):
    """order-1 zoom of the three leading axes of a [n0,n1,n2,c] to out3, float64, axis by axis (last axis first)"""
    a = np.asarray(a, dtype=np.float64)
    for k in (2, 1, 0):
        i0, i1, w, zero = axis_table(a.shape[k], out3[k])
        lo, hi = np.take(a, i0, axis=k), np.take(a, i1, axis=k)
        shp = [1, 1, 1, 1]
        shp[k] = -1
        w, zero = w.reshape(shp), zero.reshape(shp)
        # w == 0 takes the lower neighbour as it is (an upper neighbour of inf would otherwise leak through 0 * inf)
        a = np.where(zero, 0.0, np.where(w == 0, lo, (1.0 - w) * lo + w * hi))
    return a


def corner_max(a, out3):
    """max |value| over the 8 source corners of every output element: what the elementwise bound scales with"""
    m = np.abs(np.asarray(a, dtype=np.float64))
    for k in (2, 1, 0):
        i0, i1, _, _ = axis_table(m.shape[k], out3[k])
        m = np.maximum(np.take(m, i0, axis=k), np.take(m, i1, axis=k))
    return m


def slice_view(src, conv_axis, swap):
    """_View.__call__ of the loader on a copy: axis order of the slicing axis, velocity components exchanged"""
    order, pair = SLICE_AXES[conv_axis]
    a = np.array(src, copy=True)
    if order is not None:
        a = a.transpose(order)
        if swap and a.shape[3] > 3:
            for f in range(3):
                i, j = 4 * f + pair[0], 4 * f + pair[1]
                a[..., [i, j]] = a[..., [j, i]]
    return a


def add_adj_ref(v):
    """addAdjSlices: per packed frame (three of them) channel 0 of the previous / next slice, 0 at the ends"""
    n, h, w, _ = v.shape
    frames = v.reshape(n, h, w, 3, -1)
    c = frames.shape[4]
    out = np.zeros((n, h, w, 3, c + 2), dtype=v.dtype)
    out[..., :c] = frames
    out[1:, ..., c] = frames[:-1, ..., 0]
    out[:-1, ..., c + 1] = frames[1:, ..., 0]
    return out.reshape(n, h, w, -1)


BOUND = 2.0 ** -19       # times max |the 8 corner values|, elementwise


# ------------------------------------------------------------------------------------------------
# synthetic simulation directory: two sims x four frames, low 8^3 density + velocity, high 32^3 density, and the
# previous pass's output density_low_2x2 (32^3).  The density is either exactly 0 (a slab of every axis is empty) or
# at least 0.25, so that no slice mean comes near a threshold of 0.002 / 0.005.
# ------------------------------------------------------------------------------------------------
LOW, HIGH, SIMS, FRAMES = 8, 32, (3000, 3001), 4


def _density(rng, n):
    d = 0.25 + 0.75 * rng.random((n, n, n, 1))
    e = n // 4
    d[:e] = 0
    d[:, :e] = 0
    d[:, :, :e] = 0
    return d.astype(np.float32)


def write_sim_dir(root, uniio):
    rng = np.random.default_rng(77)
    for sim in SIMS:
        folder = os.path.join(str(root), "sim_%04d" % sim)
        os.makedirs(folder)
        for f in range(FRAMES):
            for name, arr in (("density_low_%04d.uni", _density(rng, LOW)),
                              ("velocity_low_%04d.uni", (rng.random((LOW, LOW, LOW, 3)) - 0.5).astype(np.float32)),
                              ("density_high_%04d.uni", _density(rng, HIGH)),
                              ("density_low_2x2_%04d.uni", _density(rng, HIGH))):
                vec3 = arr.shape[3] == 3
                head = uniio.make_header(arr.shape[2], arr.shape[1], arr.shape[0], vec3=vec3, grid_type=4 if vec3 else 1)
                uniio.writeUni(os.path.join(folder, name % f), head, arr)
    return str(root) + os.sep


def driver_argument_sets(base):
    """the FluidDataLoader arguments of the training drivers (GAN/multipassGAN-4x.py, -8x.py) at upRes 4 on write_sim_dir"""
    dens3, both3 = ["density"] * 3, ["density", "velocity"] * 3
    common = dict(print_info=0, base_path=base, base_path_y=base, numpy_seed=42, conv_slices=True, oldNamingScheme=False,
                  filename="density_low_%04d.uni", filename_index_min=0, filename_index_max=FRAMES, indices=list(SIMS),
                  data_fraction=1.0)
    return {
        # first 4x network, three coherent frames: x at the low resolution, y brought down to it along the slice axis
        "4x_first": dict(common, conv_axis=0, select_random=0.5, density_threshold=0.002, axis_scaling=[1, 1, 1, 1],
                         axis_scaling_y=[0.25, 1, 1, 1], filename_y="density_high_%04d.uni", multi_file_list=both3,
                         multi_file_idxOff=[0, 0, 1, 1, 2, 2], multi_file_list_y=dens3, multi_file_idxOff_y=[0, 1, 2]),
        # second 4x network: x zoomed to the high resolution on all axes, sliced along axis 2
        "4x_second": dict(common, conv_axis=2, select_random=0.5, density_threshold=0.002, axis_scaling=[4, 4, 4, 1],
                          axis_scaling_y=[1, 1, 1, 1], filename_y="density_high_%04d.uni", multi_file_list=both3,
                          multi_file_idxOff=[0, 0, 1, 1, 2, 2], multi_file_list_y=dens3, multi_file_idxOff_y=[0, 1, 2]),
        # its companion: density only, the previous pass's output as y
        "4x_second_prev": dict(common, conv_axis=2, select_random=0.5, density_threshold=0.002, axis_scaling=[4, 4, 4, 1],
                               axis_scaling_y=[1, 1, 1, 1], filename_y="density_low_2x2_%04d.uni", multi_file_list=dens3,
                               multi_file_idxOff=[0, 1, 2], multi_file_list_y=dens3, multi_file_idxOff_y=[0, 1, 2]),
        # later 8x network with add_adj_idcs: x zoomed along the slice axis only
        "8x_later_adj": dict(common, conv_axis=2, select_random=0.2, density_threshold=0.005, axis_scaling=[4, 1, 1, 1],
                             axis_scaling_y=[1, 1, 1, 1], add_adj_idcs=True, filename_y="density_high_%04d.uni",
                             multi_file_list=both3, multi_file_idxOff=[0, 0, 1, 1, 2, 2], multi_file_list_y=dens3,
                             multi_file_idxOff_y=[0, 1, 2]),
    }
