"""ParaView export of a solution: the .vtu / .pvtu files of the reference's PvtuExporter (post/VtkExport.hpp), written from the
SoA field storage on the device through l3k_vtk_* (include/l3k.h), and a reader of such files on the standard library.

    exporter = vtk.PvtuExporter(dmesh)                       # coordinates + topology, encoded once
    export_def = vtk.ExportDefinition("results/step_0.pvtu")
    export_def.define_field("T", [0])
    export_def.define_field("flux", [1, 2])                  # 2 or 3 rows: a 3-component vector
    exporter.export_solution(export_def, fields)             # fields: the (n_fields, ld) device tensor
"""
import base64
import ctypes as C
import struct
import xml.etree.ElementTree as ET

import numpy as np

from . import capi
from .capi import L3KError, check


class ExportDefinition:
    """ExportDefinition (post/VtkExport.hpp:16-39): a file name and named groups of 1, 2 or 3 rows of the field storage."""

    def __init__(self, file_name):
        self.file_name = str(file_name)
        self.fields = []

    def define_field(self, name, inds):
        self.fields.append((str(name), [int(i) for i in inds]))
        return self

    def _c_args(self):
        n = len(self.fields)
        names = (C.c_char_p * max(n, 1))(*[name.encode() for name, _ in self.fields])
        n_comps = (C.c_int * max(n, 1))(*[len(inds) for _, inds in self.fields])
        flat = [i for _, inds in self.fields for i in inds]
        comp_inds = (C.c_int * max(len(flat), 1))(*flat)
        return n, names, n_comps, comp_inds


def sizes(dim, order, n_elems, n_nodes):
    """l3k_vtk_sizes (host only): cells, raw and encoded bytes of Position, connectivity, offsets and types as a dict."""
    info = capi.VtkInfo()
    check(capi.load().l3k_vtk_sizes(dim, order, n_elems, n_nodes, C.byref(info)))
    return _info_dict(info)


def _info_dict(info):
    return {"dim": info.dim, "order": info.order, "n_points": info.n_points, "n_cells": info.n_cells, "n_conn": info.n_conn,
            "raw_bytes": list(info.raw_bytes), "encoded_bytes": list(info.encoded_bytes), "chunk_bytes": info.chunk_bytes,
            "store_bytes": info.store_bytes}


def _text(call):
    needed = C.c_size_t()
    check(call(None, 0, C.byref(needed)))
    buf = C.create_string_buffer(max(needed.value, 1))
    check(call(buf, needed.value, C.byref(needed)))
    return buf.raw[:needed.value]


def pvtu_text(export_def, n_ranks):
    """l3k_vtk_pvtu_text (host only): the bytes of the .pvtu file of an export."""
    n, names, n_comps, _ = export_def._c_args()
    lib = capi.load()
    return _text(lambda buf, cap, needed: lib.l3k_vtk_pvtu_text(export_def.file_name.encode(), n_ranks, n, names, n_comps, buf, cap, needed))


def vtu_header_text(export_def, n_points, n_cells, encoded_mesh_bytes):
    """l3k_vtk_vtu_header_text (host only): everything of a .vtu in front of the appended data, the leading `_` included."""
    n, names, n_comps, _ = export_def._c_args()
    lib = capi.load()
    enc = (C.c_uint64 * 4)(*encoded_mesh_bytes)
    return _text(lambda buf, cap, needed: lib.l3k_vtk_vtu_header_text(n_points, n_cells, enc, n, names, n_comps, buf, cap, needed))


def encode(ctx, payload):
    """l3k_vtk_encode: the base64 text of `uint64 byte count || payload` of a contiguous device tensor, as a uint8 device tensor."""
    import torch
    n_bytes = payload.numel() * payload.element_size()
    text = torch.empty(4 * ((8 + n_bytes + 2) // 3), dtype=torch.uint8, device=payload.device)
    check(capi.load().l3k_vtk_encode(ctx._h, payload.data_ptr() if n_bytes else None, n_bytes, text.data_ptr(), text.numel()))
    return text


class PvtuExporter:
    """PvtuExporter (post/VtkExport.hpp:41-97) of one rank's DeviceMesh: creation computes and encodes the coordinates and the sub-cell
    topology on the device; export_solution writes `<name>_<rank>.vtu` and, on rank 0, `<name>.pvtu`.  No rank talks to another.
    chunk_bytes: text bytes per chunk of the encode / copy / write pipeline (0: the default)."""

    def __init__(self, dmesh, rank=0, world=1, chunk_bytes=0):
        self.mesh, self.rank, self.world = dmesh, rank, world
        opts = capi.VtkOpts(chunk_bytes)
        self._h = C.c_void_p()
        check(capi.load().l3k_vtk_create(dmesh._h, C.byref(opts), C.byref(self._h)))

    def info(self):
        info = capi.VtkInfo()
        check(capi.load().l3k_vtk_info_get(self._h, C.byref(info)))
        return _info_dict(info)

    def export_solution(self, export_def, fields):
        """fields: contiguous float64 (n_fields, ld) device tensor (the storage l3k_update_solution fills), ld >= local nodes."""
        if fields.dim() != 2 or not fields.is_contiguous() or str(fields.dtype) != "torch.float64" or not fields.is_cuda:
            raise L3KError("fields must be a contiguous float64 (n_fields, ld) device tensor")
        n, names, n_comps, comp_inds = export_def._c_args()
        check(capi.load().l3k_vtk_export(self._h, export_def.file_name.encode(), self.rank, self.world, n, names, n_comps, comp_inds,
                                         fields.data_ptr(), fields.shape[1], fields.shape[0]))

    def __del__(self):
        if getattr(self, "_h", None) and capi is not None:
            capi.load().l3k_vtk_destroy(self._h)
            self._h = None


_DTYPES = {"Float64": "<f8", "Float32": "<f4", "UInt64": "<u8", "UInt32": "<u4", "UInt8": "u1", "Int64": "<i8", "Int32": "<i4"}


def read_vtu(path):
    """Reads a .vtu with appended base64 data and UInt64 headers (what the exporter writes).  Returns a dict: points [n, 3],
    connectivity, offsets, types, point_data {name: [n] or [n, 3]}, scalars / vectors (the active array names or None)."""
    raw = open(path, "rb").read()
    marker = raw.index(b"<AppendedData")
    start = raw.index(b"_", raw.index(b">", marker)) + 1
    end = raw.index(b"</AppendedData>", start)
    blob = raw[start:end].rstrip()
    root = ET.fromstring(raw[:start - 1].rstrip() + b"</AppendedData></VTKFile>")
    if root.get("header_type") != "UInt64" or root.get("byte_order") != "LittleEndian":
        raise ValueError("read_vtu reads little-endian files with UInt64 headers")
    piece = root.find("UnstructuredGrid/Piece")
    n_points, n_cells = int(piece.get("NumberOfPoints")), int(piece.get("NumberOfCells"))

    def array(node):
        off = int(node.get("offset"))
        n_bytes = struct.unpack("<Q", base64.b64decode(blob[off:off + 12])[:8])[0]
        text = blob[off:off + 4 * ((8 + n_bytes + 2) // 3)]
        a = np.frombuffer(base64.b64decode(text)[8:], dtype=_DTYPES[node.get("type")])
        nc = int(node.get("NumberOfComponents", "1"))
        return a.reshape(-1, nc) if nc > 1 else a

    by_name = lambda parent: {a.get("Name"): array(a) for a in piece.find(parent).findall("DataArray")}
    cells, pdata = by_name("Cells"), piece.find("PointData")
    out = {"n_points": n_points, "n_cells": n_cells, "points": array(piece.find("Points/DataArray")),
           "connectivity": cells["connectivity"], "offsets": cells["offsets"], "types": cells["types"],
           "point_data": by_name("PointData"), "scalars": pdata.get("Scalars"), "vectors": pdata.get("Vectors")}
    return out
