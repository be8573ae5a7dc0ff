"""The octree + RAHT anchor codec: `compress_anchor` / `decompress_anchor`, this project's counterpart of the reference's
`utils.compress_related("G-PCC", data, q_a, q_g, ...)` (`utils.py:505-529`: `tmc3 --transformType=0` with
`--positionQuantizationScale=q_g --qp=q_a --qpChromaOffset=-2 --mergeDuplicatedPoints=1`), so that rate / PSNR points of the
learned codec have something to stand against.  Not `tmc3` syntax, no bit-compatibility claim.

Three device parts: positions scaled by `position_scale` and rounded to the nearest cell, the points of a cell merged with
their mean colour (`voxelize.voxel_grid`); the lossless octree (`geometry.encode_geometry`); RAHT colour
(`attributes.encode_attributes`).

    container = u8 0xC1 | f64 position_scale | u32 len_geometry | geometry stream | attribute stream

Both parts may be coded against the previous frame as decoded (`compress_anchor(reference=, attributes=)`);
`compress_anchor_sequence` / `decompress_anchor_sequence` chain whole frames that way in a closed loop.

`compress_lossless` / `decompress_lossless` return a voxel cloud bit for bit: the same octree with the
lossless colour coder (`attributes.encode_attributes_lossless`), no scaling and no merging.

    container = u8 0xC2 | u32 len_geometry | geometry stream | attribute stream

Both parts may be coded against a reference cloud the decoder holds (the previous frame): `compress_lossless(reference=,
attributes=)`, and `compress_lossless_sequence` / `decompress_lossless_sequence` chain whole frames that way.  With
`global_motion=` the geometry may come out as a global-motion stream (0xA9, DESIGN.md section 7e "Global motion"); the colour
coder is then given the same warped reference, its colours carried (`motion.warp_cloud`), and the decoder reads the transform
back from the geometry stream.
"""
import math
import struct

import torch

from . import lib as L
from . import sparse as S
from .attributes import (INTER_LOSSY_MAGIC, INTER_MAGIC, WIDE_LOSSY_MAGIC, WIDE_MAGIC, decode_attributes, decode_attributes_lossless,
                         encode_attributes, encode_attributes_lossless)
from .geometry import canonical_rows, decode_geometry, encode_geometry, reference_slots, stream_search, stream_transform
from .motion import warp_cloud
from .voxelize import voxel_grid

MAGIC = 0xC1
HEADER = struct.Struct("<BdI")


def container_size(len_geometry, len_attributes):
    return HEADER.size + int(len_geometry) + int(len_attributes)


def parse_container(data):
    """(position_scale, geometry stream, attribute stream); PccError on a bad magic byte, scale or length."""
    if len(data) < HEADER.size:
        raise L.PccError("anchor stream truncated inside the header")
    magic, scale, len_g = HEADER.unpack_from(data, 0)
    if magic != MAGIC:
        raise L.PccError(f"anchor stream: magic byte {magic:#x}, this build reads {MAGIC:#x}")
    if not (math.isfinite(scale) and 0.0 < scale <= 1.0):
        raise L.PccError(f"anchor stream: position scale {scale} outside (0, 1]")
    if HEADER.size + len_g > len(data):
        raise L.PccError("anchor stream truncated inside the geometry stream")
    return scale, bytes(data[HEADER.size:HEADER.size + len_g]), bytes(data[HEADER.size + len_g:])


def scaled_voxels(cloud, position_scale):
    """The anchor's voxelisation: `voxel_grid` of xyz * position_scale (fp32) with unit cells centred on the integers, i.e.
    positions rounded half up and the colours of a cell averaged."""
    pts = cloud[:, :3].to(torch.float32)
    if position_scale != 1.0:
        pts = pts * float(position_scale)
    return voxel_grid(pts.contiguous(), cloud[:, 3:6], 1.0, origin=(-0.5, -0.5, -0.5))


@torch.no_grad()
def compress_anchor(cloud, qp, position_scale=1.0, chroma_qp_offset=-2, reference=None, attributes="intra", search=None, predict=None):
    """[N, 6] GPU cloud (xyz, rgb in [0, 1]) -> bytes.  position_scale in (0, 1]: below 1 the points are scaled first; points
    that then share a cell are merged with their mean colour.  qp, chroma_qp_offset: `attributes.encode_attributes`.
    reference: voxels IN THE SCALED DOMAIN that `decompress_anchor` will be given too (the previous frame's decoded geometry,
    say): the geometry is then coded against them where that is shorter (`geometry.encode_geometry`).  attributes: "intra" --
    colour ignores the reference; "auto" / "inter" -- the mode of `attributes.encode_attributes`, which then needs an [M, 6]
    reference of distinct scaled-domain integer voxels with rgb in [0, 1]: the previous frame AS DECODED
    (`compress_anchor_sequence` keeps that loop closed).  search: the block vectors' range, as in `geometry.encode_geometry`
    (None, 2 .. 7 or "auto"); the colour coder uses the range the geometry stream ended with, 2 where it fell back to intra.
    predict: the form of the intra colour stream, as in `attributes.encode_attributes` (None / False: 0xB3; True: 0xB9, coefficients
    predicted from the parent level -- what `tmc3 --transformType=0` does with its intra prediction on; "auto": the shorter);
    `decompress_anchor` reads either."""
    what = "compress_anchor"
    if attributes not in ("auto", "inter", "intra"):
        raise L.PccError(f"{what}: attributes {attributes!r} is not one of auto, inter, intra")
    if attributes != "intra" and not _has_colours(reference):
        raise L.PccError(f"{what}: attributes={attributes!r} needs an [M, 6] reference cloud (scaled-domain xyz, rgb in [0, 1])")
    if not torch.is_tensor(cloud) or cloud.dim() != 2 or cloud.shape[1] != 6 or cloud.shape[0] == 0:
        raise L.PccError(f"{what}: a non-empty [N, 6] cloud (xyz, rgb in [0, 1]) is required")
    if not cloud.is_cuda:
        raise L.PccError(f"{what} operates on GPU tensors only (no CPU fallback)")
    scale = float(position_scale)
    if not (math.isfinite(scale) and 0.0 < scale <= 1.0):
        raise L.PccError(f"{what}: position_scale {position_scale} outside (0, 1]")
    g = scaled_voxels(cloud, scale)
    c4 = torch.cat([torch.zeros((g.index.shape[0], 1), dtype=torch.int32, device=cloud.device), g.index], dim=1).contiguous()
    cs = S.coordset_from_coords(c4, 1)[0]                    # the grid's rows are ascending: canonical as they are
    levels = torch.round(g.attrs.to(torch.float64) * 255.0).clamp_(0, 255).to(torch.uint8)
    geometry = encode_geometry(cs, reference=reference, search=search)
    if attributes == "intra":
        colours = encode_attributes(cs, qp, chroma_qp_offset, attrs=levels, predict=predict)
    else:
        colours = encode_attributes(cs, qp, chroma_qp_offset, attrs=levels, reference=reference, mode=attributes,
                                    search=stream_search(geometry), predict=predict)
    return HEADER.pack(MAGIC, scale, len(geometry)) + geometry + colours


def _decode_anchor(data, device, reference):
    """(position scale, the decoded voxel set in the scaled domain, its uint8 levels): what `decompress_anchor` returns and what
    the next frame of a sequence is coded against both come from here."""
    scale, geometry, attributes = parse_container(data)
    inter = len(attributes) > 0 and attributes[0] in (INTER_LOSSY_MAGIC, WIDE_LOSSY_MAGIC)
    if inter and not _has_colours(reference):
        raise L.PccError("decompress_anchor: the colours are coded against a reference; an [M, 6] reference cloud is required")
    cs = decode_geometry(geometry, device, as_set=True, reference=reference)
    return scale, cs, decode_attributes(attributes, cs, reference=reference if inter else None)


def _decoded_cloud(scale, cs, levels):
    """[n, 6] float32: the set's voxels divided by the scale (1.0: the scaled domain itself) and levels / 255 (round(255 c) gives
    them back)."""
    dev = cs.device
    xyz = cs.coords()[:cs.n, 1:].to(torch.float64) / torch.tensor(scale, dtype=torch.float64, device=dev)
    rgb = levels.to(torch.float64) / torch.tensor(255.0, dtype=torch.float64, device=dev)
    return torch.cat([xyz, rgb], dim=1).to(torch.float32)


@torch.no_grad()
def decompress_anchor(data, device, reference=None):
    """bytes -> [n, 6] float32 on `device`: positions divided by the scale, colours / 255, in canonical order.  reference:
    the scaled-domain cloud `compress_anchor` was given; a stream whose colours are coded against it (magic byte 0xB4 of the
    attribute part) raises PccError when the reference has no colours."""
    return _decoded_cloud(*_decode_anchor(data, device, reference))


@torch.no_grad()
def compress_anchor_sequence(frames, qp, position_scale=1.0, chroma_qp_offset=-2, intra_period=32, search=None, predict=None):
    """Frames ([N, 6] clouds as for `compress_anchor`) -> one stream per frame, closed loop: frame i is coded on its own when
    i % intra_period == 0, else against frame i - 1 AS DECODED -- its voxels in the scaled domain and its decoded colours --
    with geometry and colour both "auto".  The encoder decodes every stream it wrote to hold what the decoder will hold.
    predict: the form of every intra colour stream (the intra frames and the intra candidates of the others), as in
    `compress_anchor`.  `decompress_anchor_sequence` returns the frames."""
    if int(intra_period) < 1:
        raise L.PccError(f"compress_anchor_sequence: intra_period {intra_period} is not positive")
    out, prev = [], None
    for i, frame in enumerate(frames):
        if i % int(intra_period) == 0:
            out.append(compress_anchor(frame, qp, position_scale, chroma_qp_offset, predict=predict))
            prev = None
        else:
            out.append(compress_anchor(frame, qp, position_scale, chroma_qp_offset, reference=prev, attributes="auto", search=search,
                                       predict=predict))
        _, cs, levels = _decode_anchor(out[-1], frame.device, prev)
        prev = _decoded_cloud(1.0, cs, levels)
    return out


@torch.no_grad()
def decompress_anchor_sequence(streams, device):
    """The streams of `compress_anchor_sequence` -> the frames, each [n, 6] float32 as `decompress_anchor` returns them."""
    out, prev = [], None
    for data in streams:
        scale, cs, levels = _decode_anchor(data, device, prev)
        prev = _decoded_cloud(1.0, cs, levels)                 # the reference stays in the scaled domain
        out.append(_decoded_cloud(scale, cs, levels))
    return out


# ---- the lossless codec --------------------------------------------------------------------------------------------------
LOSSLESS_MAGIC = 0xC2
LOSSLESS_HEADER = struct.Struct("<BI")


def parse_lossless_container(data):
    """(geometry stream, attribute stream); PccError on a bad magic byte or length."""
    if len(data) < LOSSLESS_HEADER.size:
        raise L.PccError("lossless stream truncated inside the header")
    magic, len_g = LOSSLESS_HEADER.unpack_from(data, 0)
    if magic != LOSSLESS_MAGIC:
        raise L.PccError(f"lossless stream: magic byte {magic:#x}, this build reads {LOSSLESS_MAGIC:#x}")
    if LOSSLESS_HEADER.size + len_g > len(data):
        raise L.PccError("lossless stream truncated inside the geometry stream")
    return bytes(data[LOSSLESS_HEADER.size:LOSSLESS_HEADER.size + len_g]), bytes(data[LOSSLESS_HEADER.size + len_g:])


def _first_cloud(reference, what):
    """The cloud the colour coder sees of a `reference=` argument: the argument itself, or the first entry's cloud of a list."""
    return reference_slots(reference, what)[0][0] if isinstance(reference, (list, tuple)) else reference


def _has_colours(reference):
    return torch.is_tensor(reference) and reference.dim() == 2 and reference.shape[1] == 6


@torch.no_grad()
def _colour_reference(reference, geometry):
    """The reference the colour coder sees: the one given, or -- behind a global-motion geometry stream -- that reference
    warped by the stream's transform with its colours carried, the cloud the geometry's block search ran against."""
    T = stream_transform(geometry)
    if T is None:
        return reference
    # the colour coder refuses a reference whose rows repeat a voxel; the warp would merge them silently, so it is refused here
    # as well: what a malformed reference does must not depend on whether the geometry came out wrapped
    rs, _, keep = canonical_rows(reference, "lossless codec (reference)")
    if keep is not None:
        raise L.PccError(f"lossless codec (reference): {reference.shape[0] - rs.n} rows repeat a voxel; merge them first (voxelize.voxel_grid)")
    return warp_cloud(reference, T)


@torch.no_grad()
def compress_lossless(cloud, reference=None, attributes="intra", global_motion=None, search=None):
    """[N, 6] GPU cloud of distinct voxels (integer xyz, rgb in [0, 1]: colours become round(255 c)) -> bytes from which
    `decompress_lossless` returns the same voxels with the same levels.  Non-integer coordinates and repeated voxels raise
    PccError: voxelise first (`voxelize.voxel_grid`).  reference: a voxel cloud (its first three columns) the decoder holds
    too, e.g. the previous frame: the geometry is coded against it where that is shorter.  attributes: "intra" -- the colours
    ignore the reference; "auto" / "inter" -- the mode of `attributes.encode_attributes_lossless`, which then needs an [M, 6]
    reference of distinct voxels and codes the colours against its colours.  global_motion: as in
    `geometry.encode_geometry` (None, "auto" or a RigidTransform); when the geometry comes out wrapped, the colours are coded
    against the warped reference.  search: the block vectors' range, as in `geometry.encode_geometry` (None, 2 .. 7 or "auto");
    the colour coder uses the range the geometry stream ended with, 2 where it fell back to intra.
    reference may also be a list of 1..4 clouds or pairs (cloud, RigidTransform), as `geometry.encode_geometry` takes them
    (global_motion must then be None): the geometry chooses among them per block, the colours see the first entry's cloud,
    plain, exactly as if it were the only reference."""
    what = "compress_lossless"
    if attributes not in ("auto", "inter", "intra"):
        raise L.PccError(f"{what}: attributes {attributes!r} is not one of auto, inter, intra")
    references, reference = reference, _first_cloud(reference, what)
    if attributes != "intra" and not _has_colours(reference):
        raise L.PccError(f"{what}: attributes={attributes!r} needs an [M, 6] reference cloud (xyz, rgb in [0, 1])")
    if not torch.is_tensor(cloud) or cloud.dim() != 2 or cloud.shape[1] != 6 or cloud.shape[0] == 0:
        raise L.PccError(f"{what}: a non-empty [N, 6] cloud (xyz, rgb in [0, 1]) is required")
    if not cloud.is_cuda:
        raise L.PccError(f"{what} operates on GPU tensors only (no CPU fallback)")
    xyz = cloud[:, :3]
    if xyz.dtype.is_floating_point and not bool((xyz == torch.floor(xyz)).all()):
        raise L.PccError(f"{what}: coordinates are not integers; voxelise the cloud first (voxelize.voxel_grid)")
    c4 = torch.cat([torch.zeros((cloud.shape[0], 1), dtype=torch.int32, device=cloud.device), xyz.to(torch.int32)], dim=1).contiguous()
    cs, perm, keep = S.coordset_from_coords(c4, 1)
    if keep is not None:
        raise L.PccError(f"{what}: {cloud.shape[0] - cs.n} rows repeat a voxel; merge them first (voxelize.voxel_grid)")
    levels = torch.round(cloud[:, 3:6].to(torch.float64) * 255.0).clamp_(0, 255).to(torch.uint8)
    levels = (levels if perm is None else levels[perm]).contiguous()
    geometry = encode_geometry(cs, reference=references, global_motion=global_motion, search=search)
    if attributes == "intra":
        colours = encode_attributes_lossless(cs, attrs=levels)
    else:
        colours = encode_attributes_lossless(cs, attrs=levels, reference=_colour_reference(reference, geometry), mode=attributes,
                                             search=stream_search(geometry))
    return LOSSLESS_HEADER.pack(LOSSLESS_MAGIC, len(geometry)) + geometry + colours


@torch.no_grad()
def decompress_lossless(data, device, reference=None):
    """bytes -> [n, 6] float32 on `device` in canonical order: the exact coordinates, colours level / 255 (round(255 c) of
    them gives the levels back).  reference: the cloud `compress_lossless` was given; a stream whose colours are coded against
    it (magic byte 0xB6 of the attribute part) raises PccError when the reference has no colours.  A list, as
    `compress_lossless` took it, goes to the geometry decoder; the colours see its first entry's cloud."""
    geometry, attributes = parse_lossless_container(data)
    references, reference = reference, _first_cloud(reference, "decompress_lossless")
    inter = len(attributes) > 0 and attributes[0] in (INTER_MAGIC, WIDE_MAGIC)
    if inter and not _has_colours(reference):
        raise L.PccError("decompress_lossless: the colours are coded against a reference; an [M, 6] reference cloud is required")
    cs = decode_geometry(geometry, device, as_set=True, reference=references)
    levels = decode_attributes_lossless(attributes, cs, reference=_colour_reference(reference, geometry) if inter else None)
    rgb = levels.to(torch.float64) / torch.tensor(255.0, dtype=torch.float64, device=cs.device)
    return torch.cat([cs.coords()[:cs.n, 1:].to(torch.float64), rgb], dim=1).to(torch.float32)


@torch.no_grad()
def compress_lossless_sequence(frames, intra_period=32, global_motion=None, search=None, references=1):
    """Frames ([N, 6] clouds as for `compress_lossless`) -> one stream per frame: frame i is coded on its own when
    i % intra_period == 0, else against frame i - 1 with geometry and colour both "auto" (lossless: the decoder holds the same
    frame) and `global_motion` as given.  Every stream decodes with `decompress_lossless(stream, device, reference=previous
    frame)`.  references=2: a frame whose two predecessors both lie inside its intra period codes its geometry against
    [frame i - 1, frame i - 2] (global_motion must then be None) and decodes with that list; its colours see frame i - 1."""
    if int(intra_period) < 1:
        raise L.PccError(f"compress_lossless_sequence: intra_period {intra_period} is not positive")
    if references not in (1, 2) or (references == 2 and global_motion is not None):
        raise L.PccError("compress_lossless_sequence: references is 1 or 2, and 2 goes with global_motion=None")
    out, prev, prev2 = [], None, None
    for i, frame in enumerate(frames):
        at = i % int(intra_period)
        if at == 0:
            out.append(compress_lossless(frame))
        elif references == 2 and at >= 2:
            out.append(compress_lossless(frame, reference=[prev, prev2], attributes="auto", search=search))
        else:
            out.append(compress_lossless(frame, reference=prev, attributes="auto", global_motion=global_motion, search=search))
        prev, prev2 = frame, prev
    return out


@torch.no_grad()
def decompress_lossless_sequence(streams, device):
    """The streams of `compress_lossless_sequence` -> the frames, each [n, 6] float32 in canonical order."""
    out, prev, prev2 = [], None, None
    for data in streams:
        prev, prev2 = decompress_lossless(data, device, reference=[prev, prev2] if prev2 is not None else prev), prev
        out.append(prev)
    return out
