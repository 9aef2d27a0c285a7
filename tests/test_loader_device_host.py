"""What the device loader (multi-pass-gan_amd/fluiddataloader_device.py) decides on the host, held against the unmodified
FluidDataLoader, and the float64 restatement of its kernels (tests/loader_device_ref.py) held against scipy.  No GPU."""
import os
import sys

import numpy as np
import pytest
import scipy.ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import loader_device_ref as R  # noqa: E402

# source shape, factors: the cases of the GPU test, the drivers' ratios, and sizes whose last coordinate
# (big - 1) * ((n - 1) / (big - 1)) rounds above n - 1 (scipy writes 0 there)
ZOOM_CASES = [((5, 6, 7, 4), (2, 3, 1)), ((4, 4, 4, 12), (4, 4, 4)), ((8, 6, 7, 3), (0.25, 1, 1)), ((1, 6, 7, 4), (1, 2, 2)),
              ((3, 5, 5, 4), (8, 1, 1)), ((8, 8, 8, 2), (4, 4, 4)), ((16, 3, 3, 1), (4, 1, 1)), ((32, 4, 3, 1), (0.25, 1, 1)),
              ((6, 7, 50, 1), (1, 1, 3.9)), ((7, 7, 7, 2), (0.5, 1.5, 2.5))]


@pytest.mark.parametrize("shape,factors", ZOOM_CASES)
def test_restatement_agrees_with_scipy(shape, factors):
    rng = np.random.default_rng(3)
    a = rng.random(shape)
    want = scipy.ndimage.zoom(a, list(factors) + [1], order=1)
    out3 = [R.out_size(n, f) for n, f in zip(shape, factors)]
    assert list(want.shape[:3]) == out3
    got = R.zoom_ref(a, out3)
    err = float(np.max(np.abs(got - want)))
    print("max |restatement - scipy| = %.3e" % err)
    assert err <= 1e-15
    # factor 1 on every axis is the array itself
    assert np.array_equal(R.zoom_ref(a, shape[:3]), a)
    # the bound's scale really bounds the result
    assert np.all(np.abs(got) <= R.corner_max(a, out3))


def test_restatement_covers_the_zeroed_last_index():
    """the search that found a size where scipy's last coordinate leaves the array: the restatement zeroes it too"""
    hits = [(n, big) for n in range(2, 70) for big in range(2, 300)
            if (big - 1) * (float(n - 1) / float(big - 1)) > n - 1]
    assert hits, "no such size below 70 -> 300"
    n, big = hits[0]
    a = 1.0 + np.random.default_rng(4).random((n, 2, 2, 1))
    want = scipy.ndimage.zoom(a, [big / n, 1, 1, 1], order=1)
    assert want.shape[0] == big and np.all(want[-1] == 0)
    assert np.max(np.abs(R.zoom_ref(a, [big, 2, 2]) - want)) <= 1e-15


@pytest.mark.parametrize("conv_axis", [0, 1, 2])
@pytest.mark.parametrize("channels", [1, 3, 12])
def test_slice_view_plan_is_the_loaders_view(mpg, conv_axis, channels):
    from mpgan_amd import fluiddataloader as FDL
    from mpgan_amd.fluiddataloader_device import slice_view_plan

    class L(object):
        conv_slices, collapse_z = True, False

        def removeZComponent(self, x):
            return x
    L.conv_axis = conv_axis
    a = np.random.default_rng(5).random((3, 4, 5, channels)).astype(np.float32)
    for swap in (True, False):
        want = FDL._View(L(), swap, None)(a.copy())
        perm, cmap = slice_view_plan(conv_axis, swap, channels)
        got = (a if perm is None else a.transpose(tuple(perm) + (3,)))[..., cmap]
        assert np.array_equal(got, want)
        assert np.array_equal(R.slice_view(a, conv_axis, swap), want)


def test_zoomed_size_is_scipys(mpg):
    from mpgan_amd.fluiddataloader_device import zoomed_size
    for shape, factors in ZOOM_CASES:
        want = scipy.ndimage.zoom(np.zeros(shape), list(factors) + [1], order=1).shape[:3]
        assert tuple(zoomed_size(shape[:3], factors)) == want


@pytest.fixture(scope="module")
def sim_dir(tmp_path_factory):
    import mpgan_amd  # noqa: F401
    from mpgan_amd import uniio
    return R.write_sim_dir(tmp_path_factory.mktemp("loader_sims"), uniio)


@pytest.mark.parametrize("name", ["4x_first", "4x_second", "4x_second_prev", "8x_later_adj"])
def test_planning_reproduces_the_host_loader(mpg, sim_dir, name):
    """The host loader's result rebuilt from the device loader's planning functions, with scipy standing in for the
    kernels: kept indices from the vector of means, truncation, the random draw."""
    from mpgan_amd import fluiddataloader as FDL
    from mpgan_amd.fluiddataloader_device import kept_slices, select_rows, slice_view_plan, zoomed_size
    kw = R.driver_argument_sets(sim_dir)[name]
    host = FDL.FluidDataLoader(**kw)
    state = np.random.get_state()
    hx, hy, _ = host.get()
    assert hx.shape[0] == hy.shape[0] > 0

    np.random.seed(kw["numpy_seed"])
    rows_x, rows_y = [], []
    for e in host._entries:
        ax = host._assemble(e.x, kw["multi_file_list"], kw["multi_file_idxOff"], "arr_0")
        ay = host._assemble(e.y, kw["multi_file_list_y"], kw["multi_file_idxOff_y"], "arr_0")
        perm, cmap = slice_view_plan(kw["conv_axis"], True, ax.shape[3])
        t = (0, 1, 2, 3) if perm is None else tuple(perm) + (3,)
        vx, vy = ax.transpose(t)[..., cmap], ay.transpose(t)
        fx = scipy.ndimage.zoom(vx, kw["axis_scaling"], order=1)
        fy = scipy.ndimage.zoom(vy, kw["axis_scaling_y"], order=1)
        assert list(fx.shape[:3]) == zoomed_size(vx.shape[:3], kw["axis_scaling"][:3])
        assert list(fy.shape[:3]) == zoomed_size(vy.shape[:3], kw["axis_scaling_y"][:3])
        means = [np.average(fx[s, :, :, 0:1]) for s in range(fx.shape[0])]
        # the directory was built so that no decision hangs on rounding
        thr = kw["density_threshold"]
        assert all(abs(float(m) - thr) > 1e-4 * thr for m in means)
        keep = kept_slices(means, thr)
        assert keep == host._dense_enough(fx)
        assert 0 < len(keep) < fx.shape[0]
        keep = select_rows(keep, kw["select_random"])
        if kw.get("add_adj_idcs"):
            fx = R.add_adj_ref(fx)
        rows_x.append(fx[keep])
        rows_y.append(fy[keep])
    assert np.array_equal(np.concatenate(rows_x), hx)
    assert np.array_equal(np.concatenate(rows_y), hy)
    after = np.random.get_state()
    assert after[0] == state[0] and np.array_equal(after[1], state[1]) and after[2:] == state[2:]


def test_uncovered_arguments_run_the_parents_code(mpg, sim_dir):
    """conv_slices=False is not the device path's: the subclass returns the parent's arrays, and needs no GPU for it"""
    from mpgan_amd import fluiddataloader as FDL
    from mpgan_amd.fluiddataloader_device import DeviceFluidDataLoader
    kw = dict(print_info=0, base_path=sim_dir, base_path_y=sim_dir, numpy_seed=7, filename="density_low_%04d.uni",
              filename_y="density_high_%04d.uni", filename_index_min=0, filename_index_max=R.FRAMES, indices=list(R.SIMS),
              multi_file_list=["density", "velocity"], multi_file_list_y=["density"])
    host = FDL.FluidDataLoader(**kw)
    state = np.random.get_state()
    dev = DeviceFluidDataLoader(device="cuda:0", **kw)
    assert not dev.used_device_path
    assert np.array_equal(dev.get()[0], host.get()[0]) and np.array_equal(dev.get()[1], host.get()[1])
    assert dev.get()[2] == host.get()[2]
    after = np.random.get_state()
    assert after[0] == state[0] and np.array_equal(after[1], state[1])
    # slice mode with add_adj_idcs but without y keeps the parent's error
    with pytest.raises(FDL.FluidDataLoaderError):
        DeviceFluidDataLoader(device="cuda:0", conv_slices=True, add_adj_idcs=True, **dict(kw, filename_y=None,
                                                                                          multi_file_list_y=None))
