"""``FluidDataLoader`` slice mode with the array work in HIP kernels (csrc/mpgan_loader.hip).

The host loader (``fluiddataloader.loadFiles``, the reference's tools_wscale/fluiddataloader.py:387-544) zooms every
entry to its full size with ``scipy.ndimage.zoom`` on one thread -- [64,64,64,12] -> [256,256,256,12], 0.8 GB, for the
second 4x network -- takes the per-slice density means of the result, and then keeps 10-40 % of the slices.  Here an
entry's source is uploaded once; ``mpg_slice_zoom_means`` returns the means of the zoomed array without storing it,
and ``mpg_slice_zoom_gather`` interpolates the kept slices only (the slice-axis view, the exchange of velocity
components, both zooms, ``addAdjSlices`` and the row selection in one launch per source).  The files of a multi-file
y entry (three 512^3 frames for the 8x networks) are uploaded one at a time and written into their channel windows.

What stays on the host, in the parent's order: file enumeration and ``.uni`` decoding, the storage sized by
``select_random`` before filtering, the comparison of the means with ``density_threshold``, the
``np.random.shuffle(np.arange(kept))`` draw (the numpy generator ends in the parent's state) and the truncation of
paired slice sets.  A slice whose mean density sits within float rounding of the threshold can be decided differently
from the host path (fp32 block sums here, numpy's pairwise sum there); everything else agrees to fp32 interpolation
rounding, and bit for bit where the zoom factors are 1.

What the device path does not cover runs the parent's code unchanged: ``conv_slices=False``, ``shape`` / ``shape_y``
resizing, ``postproc_func*``, ``array_y`` / ``func_y``, ``.npz`` payloads, ``collapse_z``, unpaired slice sets, a
channel factor other than 1.
"""
import ctypes
import warnings

import numpy as np

from . import _lib
from .fluiddataloader import FluidDataLoader, FluidDataLoaderError, _View

MEANS_WS_PER_SLICE = 64         # floats of workspace per slice mpg_slice_zoom_means asks for (include/mpgan.h)
MAX_CHANNELS = 16               # mapped channels of one mpg_slice_zoom_gather


def _ints(vals):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


# ------------------------------------------------------------------------------------------------
# host-side planning (no GPU): shapes, channel maps, which slices are kept
# ------------------------------------------------------------------------------------------------
def zoomed_size(shape3, factors3):
    """scipy.ndimage.zoom's output size"""
    return [int(round(n * f)) for n, f in zip(shape3, factors3)]


def slice_view_plan(conv_axis, swap, channels):
    """-> (perm3 or None, chan_map): V[.., q] = transpose(src, perm)[.., chan_map[q]]  (_View.__call__, :416-431)"""
    order, pair = _View.SLICE_AXES[conv_axis]
    cmap = list(range(channels))
    if order is None:
        return None, cmap
    if swap and channels > 3:
        for f in range(3):
            i, j = 4 * f + pair[0], 4 * f + pair[1]
            cmap[i], cmap[j] = cmap[j], cmap[i]
    return list(order[:3]), cmap


def kept_slices(means, density_threshold):
    """_dense_enough on the vector of slice means"""
    return [i for i in range(len(means)) if float(means[i]) >= density_threshold]


def select_rows(keep, select_random):
    """selectRandomSamples on paired data: the draw whose permutation is discarded, then the first int(n * select_random)"""
    np.random.shuffle(np.arange(len(keep)))
    return keep[:int(len(keep) * select_random)]


# ------------------------------------------------------------------------------------------------
# thin wrappers of the C ABI
# ------------------------------------------------------------------------------------------------
def _check_source(src):
    import torch
    if not (src.is_cuda and src.dtype == torch.float32 and src.dim() == 4 and src.is_contiguous()):
        raise ValueError("source: a contiguous float32 device tensor [d0,d1,d2,c], got %s %s" % (src.dtype, tuple(src.shape)))


def slice_zoom_means(src, perm, out3, chan=0):
    """src [d0,d1,d2,c] (device, fp32) -> means over (i, j) of zoom(transpose(src, perm))[s, i, j, chan], [out3[0]] (device)"""
    import torch
    from .ops import _ptr, _stream
    lib = _lib.load()
    _check_source(src)
    means = torch.empty(int(out3[0]), dtype=torch.float32, device=src.device)
    ws = torch.empty(MEANS_WS_PER_SLICE * int(out3[0]), dtype=torch.float32, device=src.device)
    _lib.check(lib.mpg_slice_zoom_means(_stream(), _ptr(src), _ints(src.shape[:3]), int(src.shape[3]),
                                        None if perm is None else _ints(perm), _ints(out3), int(chan), _ptr(means), _ptr(ws),
                                        ws.numel()), "mpg_slice_zoom_means")
    return means


def slice_zoom_gather(src, perm, out3, slices, chan_map, out, c_off=0, adj=False):
    """out[r, i, j, c_off + q] = zoom(transpose(src, perm))[slices[r], i, j, chan_map[q]]; slices: int32 device tensor;
    out [len(slices), out3[1], out3[2], out_c] (device, fp32).  adj: see include/mpgan.h."""
    import torch
    from .ops import _ptr, _stream
    lib = _lib.load()
    _check_source(src)
    if not (slices.is_cuda and slices.dtype == torch.int32 and slices.is_contiguous() and out.is_cuda
            and out.dtype == torch.float32 and out.dim() == 4):
        raise ValueError("slice_zoom_gather: slices int32, out float32 [k,h,w,c], both on the device")
    if tuple(out.shape[:3]) != (slices.numel(), int(out3[1]), int(out3[2])) or not out.is_contiguous():
        raise ValueError("slice_zoom_gather: out %s for %d slices of %s" % (tuple(out.shape), slices.numel(), list(out3)))
    cmap = list(range(src.shape[3])) if chan_map is None else list(chan_map)
    _lib.check(lib.mpg_slice_zoom_gather(_stream(), _ptr(src), _ints(src.shape[:3]), int(src.shape[3]),
                                         None if perm is None else _ints(perm), _ints(out3), _ptr(slices), slices.numel(),
                                         _ints(cmap), len(cmap), int(bool(adj)), _ptr(out), int(out.shape[3]), int(c_off)),
               "mpg_slice_zoom_gather")
    return out


# ------------------------------------------------------------------------------------------------
class DeviceFluidDataLoader(FluidDataLoader):
    """``FluidDataLoader(...)`` plus ``device=``; ``get()`` as the parent, ``get_device()`` the same data as CUDA tensors"""

    def __init__(self, *args, device="cuda:0", **kw):
        self.device = device
        self.used_device_path = False
        self._dev = None
        super().__init__(*args, **kw)

    def _device_path_applies(self):
        names = [self.filename, self.filename_y]
        return bool(self.conv_slices and self.have_y_npz and self.shape is None and self.shape_y is None
                    and self.postproc_func is None and self.postproc_func_y is None and self.array_y is None
                    and self.func_y is None and not self.collapse_z and self.wildcard is None
                    and all(n is not None and n.endswith(".uni") for n in names)
                    and float(self.axis_scaling[3]) == 1.0 and float(self.axis_scaling_y[3]) == 1.0)

    def _parts(self, first, names, offsets):
        """the grids `_assemble` would concatenate, one at a time"""
        shift = (lambda i: 0) if offsets is None else (lambda i: offsets[i])
        yield self.loadSingleDatum(first, self.np_load_string_y, shift(0))
        if names is not None:
            if names[0] not in first:
                raise FluidDataLoaderError("Error, input filename '%s' doesnt contain given string '%s'" % (first, names[0]))
            for i in range(1, len(names)):
                yield self.loadSingleDatum(first.replace(names[0], names[i]), self.np_load_string_y, shift(i))

    def _upload(self, a):
        import torch
        with warnings.catch_warnings():      # readUni returns a read-only view of the file's bytes; it is only read here
            warnings.simplefilter("ignore", UserWarning)
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)

    def loadFiles(self):
        if not self._device_path_applies():
            return super().loadFiles()
        import torch
        n = len(self._entries)
        self.do_zoom = False
        filled = 0
        for e in self._entries:
            ax = self._assemble(e.x, self.multi_file_list, self.multi_file_idxOff, self.np_load_string)
            parts_y = self._parts(e.y, self.multi_file_list_y, self.multi_file_idxOff_y)
            y0 = next(parts_y)
            cx = ax.shape[-1]
            # the parent's own errors (a velocity exchange on fewer than three packed frames, adjacent slices of
            # channels that are not three frames) stay the parent's
            if (ax.ndim != 4 or y0.ndim != 4 or cx > MAX_CHANNELS or (self.conv_axis != 0 and 3 < cx < 12)
                    or (self.add_adj_idcs and cx % 3 != 0)):
                if self.x is not None:
                    raise FluidDataLoaderError("entries of one loader differ in what the device path covers")
                return super().loadFiles()
            perm, cmap_x = slice_view_plan(self.conv_axis, True, cx)
            view = (lambda s: s) if perm is None else (lambda s: tuple(s[k] for k in perm))
            vx_shape = view(ax.shape[:3]) + (ax.shape[3],)
            cy = y0.shape[3] * (1 if self.multi_file_list_y is None else len(self.multi_file_list_y))
            vy_shape = view(y0.shape[:3]) + (cy,)
            if self.x is None:                       # the first sample fixes the storage, as in the parent
                self.data_shape = vx_shape
                self.shape = vx_shape * np.asarray(self.axis_scaling)
                if self.add_adj_idcs:
                    self.shape[3] += 6
                self.x = self._allocate(n * self.shape[0] * self.select_random, self.shape[1:])
                if self.print_info:
                    print("x storage %s for %d entries of shape %s" % (self.x.shape, n, list(self.shape)))
                self.data_shape_y = vy_shape * np.asarray(self.axis_scaling_y)
                self.shape_y = vy_shape
                self.y = self._allocate(self.x.shape[0], self.shape_y[1:])
            ox = zoomed_size(vx_shape[:3], self.axis_scaling[:3])
            oy = zoomed_size(vy_shape[:3], self.axis_scaling_y[:3])
            src = self._upload(ax)
            means = slice_zoom_means(src, perm, ox, 0).cpu().numpy()
            keep = kept_slices(means, self.density_threshold)
            if keep and keep[-1] >= oy[0]:
                raise IndexError("index %d is out of bounds for axis 0 with size %d" % (keep[-1], oy[0]))
            keep = select_rows(keep, self.select_random)
            k = len(keep)
            if k:
                table = torch.as_tensor(np.asarray(keep, dtype=np.int32)).to(self.device)
                gx = torch.empty((k, ox[1], ox[2], ax.shape[3] + (6 if self.add_adj_idcs else 0)), dtype=torch.float32,
                                 device=self.device)
                slice_zoom_gather(src, perm, ox, table, cmap_x, gx, 0, self.add_adj_idcs)
                self.x[filled:filled + k, :] = gx.cpu().numpy()
                del src, gx
                gy = torch.empty((k, oy[1], oy[2], cy), dtype=torch.float32, device=self.device)
                c_off, part = 0, y0
                while part is not None:              # one file in HBM at a time, each into its channel window
                    if part.shape != y0.shape:
                        raise FluidDataLoaderError("y grids of one entry differ in shape: %s, %s" % (part.shape, y0.shape))
                    slice_zoom_gather(self._upload(part), perm, oy, table, None, gy, c_off, False)
                    c_off += part.shape[3]
                    part = next(parts_y, None)
                self.y[filled:filled + k, :] = gy.cpu().numpy()
                del gy
            filled += k
        self.used_device_path = True
        if self.print_info:
            print("kept %d of %d slice slots (density_threshold %s, select_random %s)"
                  % (filled, self.x.shape[0], self.density_threshold, self.select_random))
        self.x = self.x[:filled]
        self.y = self.y[:filled]

    def get_device(self):
        """-> (x, y, filenames) with x and y as tensors on `device` (uploaded on first use; y may be a list of labels)"""
        import torch
        if self._dev is None:
            up = lambda a: torch.as_tensor(a).to(self.device) if isinstance(a, np.ndarray) else a    # noqa: E731
            self._dev = (up(self.x), up(self.y))
        return self._dev[0], self._dev[1], self.xfn
