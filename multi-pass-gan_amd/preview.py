"""Preview images of the inference drivers: what the reference writes next to its .uni volumes.

``save_img_3d`` (multipassGAN-out.py:208-210; called at :461,523,585, multipassGAN-4x.py:1134,1146 and
multipassGAN-8x.py:1718) stacks the three axis sums of ``dim_output / 80``; the slice loop (-out.py:592-604) writes the two
mid planes along every axis, gated on the mean of the xy plane, and every plane of frame 110.  Both look at the volume
BEFORE the ``< 5e-4`` cutoff, which here is fused into the final transpose -- so the pictures are taken from the pass
volumes in HBM (``ops.volume_projections`` / ``volume_planes_gray8`` / ``gray8``) and only bytes reach the host.

A pass hands over its volume as it lies in memory together with ``perm``: the reference's ``dim_output`` at that line
is ``vol.permute(perm)``.  Axis sums and planes commute with the permutation, so the volume itself is never transposed.
"""
import os
import sys

import numpy as np
import torch

from . import heldout, ops

GATE = 0.0001                   # multipassGAN-out.py:595,601
DUMP_FRAME = 110                # :599
KINDS = ("slice_xy", "slice_yz", "slice_xz")
# plane i of dim_output's axis, stored transposed or not: dim_output[i], .transpose(2,1,0)[i], .transpose(1,0,2)[i]  (:596-598)
_KIND_PLANE = {"slice_xy": (0, False), "slice_yz": (2, True), "slice_xz": (1, False)}


def _perm(perm):
    perm = tuple(int(p) for p in perm)
    if sorted(perm) != [0, 1, 2]:
        raise ValueError("perm %r is not a permutation of (0, 1, 2)" % (perm,))
    return perm


def plane_of(perm, axis, transposed):
    """plane i of axis `axis` of vol.permute(perm) (transposed or not) -> (axis, transposed) of the same image taken from vol"""
    rest = [perm[d] for d in range(3) if d != axis]
    return perm[axis], bool(transposed) != (rest[0] > rest[1])


def projection_image(vol, perm=(0, 1, 2), divisor=80.0):
    """the uint8 [B + A + A, C] image save_img_3d makes of vol.permute(perm) / divisor, vol.permute(perm) being [A, B, C]"""
    perm = _perm(perm)
    sums = ops.volume_projections(vol, divisor)
    rows = []
    for axis in range(3):
        v_axis, swap = plane_of(perm, axis, False)
        rows.append(sums[v_axis].t() if swap else sums[v_axis])
    if len(set(r.shape[1] for r in rows)) != 1:
        raise ValueError("projection_image: the three sums of a %s volume have different widths" %
                         (tuple(vol.shape[p] for p in perm),))
    return ops.gray8(torch.cat(rows, dim=0).contiguous())


def slice_images(vol, perm, indices):
    """{kind: [(i, uint8 image)]} for i in indices: the planes the reference's slice loop saves of vol.permute(perm).  The
    mean of the xy plane gates all three files of an index (:595-598).  Synchronises once, for the means."""
    perm = _perm(perm)
    indices = [int(i) for i in indices]
    out = {kind: [] for kind in KINDS}
    if not indices:
        return out
    axis, tr = plane_of(perm, *_KIND_PLANE["slice_xy"])
    gray, mean = ops.volume_planes_gray8(vol, axis, indices, tr)
    keep = [t for t, m in enumerate(mean.cpu().numpy()) if float(m) > GATE]
    if not keep:
        return out
    kept = [indices[t] for t in keep]
    out["slice_xy"] = [(indices[t], gray[t]) for t in keep]
    for kind in ("slice_yz", "slice_xz"):
        axis, tr = plane_of(perm, *_KIND_PLANE[kind])
        g, _ = ops.volume_planes_gray8(vol, axis, kept, tr)
        out[kind] = [(i, g[t]) for t, i in enumerate(kept)]
    return out


def _host(img):
    return img.cpu().numpy() if hasattr(img, "cpu") else np.asarray(img)


class PreviewSink(object):
    """Collects the pictures of one frame and writes them under the reference's names into out_dir.

    The passes call ``projection(tag, vol, perm)`` where the reference calls save_img_3d (tag "1st" / "2nd" / "3rd" for
    source_1st_%04d.png ..., None for source_%04d.png) and ``slices(vol, perm)`` where its slice loop runs: the planes
    size // 2 - 1 and size // 2 as slice_xy_<i>_<frame>.png ..., and for frame 110 the planes 0 .. tile_size_high - 1 under
    the swapped names slice_xy_<frame>_<i>.png (:600-604; the bound is tileSizeHigh, not simSizeHigh).
    ``images``: the module that makes the images (this one; the tests feed numpy images through a stub)."""

    def __init__(self, out_dir, frame_no, tile_size_high, images=None):
        self.out_dir, self.frame_no, self.tile_size_high = str(out_dir), int(frame_no), int(tile_size_high)
        self.images = sys.modules[__name__] if images is None else images
        self.written = []

    def check_comm(self, comm):
        """a rank holds only its slab of a pass volume, and the drivers run one process per volume"""
        if comm is not None and comm.world > 1:
            raise ValueError("previews are taken in one process (world %d): a rank holds only its slab" % comm.world)

    def _write(self, name, img):
        img = _host(img)
        with open(os.path.join(self.out_dir, name), "wb") as f:
            f.write(heldout.encode_gray_png(img))
        self.written.append(name)

    def projection(self, tag, vol, perm=(0, 1, 2)):
        name = "source_%04d.png" % self.frame_no if tag is None else "source_%s_%04d.png" % (tag, self.frame_no)
        self._write(name, self.images.projection_image(vol, perm, 80.0))

    def slices(self, vol, perm=(0, 1, 2)):
        size = int(vol.shape[_perm(perm)[0]])
        mid = self.images.slice_images(vol, perm, range(size // 2 - 1, size // 2 + 1))
        for kind in KINDS:
            for i, img in mid[kind]:
                self._write("%s_%04d_%04d.png" % (kind, i, self.frame_no), img)
        if self.frame_no == DUMP_FRAME:
            dump = self.images.slice_images(vol, perm, range(0, self.tile_size_high))
            for kind in KINDS:
                for i, img in dump[kind]:
                    self._write("%s_%04d_%04d.png" % (kind, self.frame_no, i), img)
