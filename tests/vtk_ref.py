"""A numpy + standard-library restatement of the ParaView export: the complete expected bytes of a .vtu and a .pvtu from a
partition's host arrays (file layout: include/l3k.h, after the reference's post/VtkExport.hpp).  Connectivity by the sub-cell rule,
coordinates from part.node_coords(), fields from a host copy, text from base64.b64encode.  No library code."""
import base64
import os
import struct

import numpy as np


def encoded(payload):
    """one array: base64 of `uint64 byte count || payload`"""
    payload = bytes(payload)
    return base64.b64encode(struct.pack("<Q", len(payload)) + payload)


def encoded_len(n_bytes):
    return 4 * ((8 + n_bytes + 2) // 3)


def topology(elem_nodes, dim, order):
    """(connectivity uint32 [n_cells * 2^dim], offsets uint32 [n_cells], types uint8 [n_cells]): p^dim linear cells per element over its
    lexicographic node grid, elements in mesh order, sub-cells layer / row / column; vertices base, +1, +n+1, +n (hexes: then the same
    four one layer up)"""
    p, n = order, order + 1
    base = np.array([layer * n * n + row * n + col for layer in range(p if dim == 3 else 1) for row in range(p) for col in range(p)])
    corner = [0, 1, n + 1, n]
    if dim == 3:
        corner = corner + [c + n * n for c in corner]
    local = base[:, None] + np.asarray(corner)[None, :]  # [p^dim][2^dim] local node numbers
    conn = np.asarray(elem_nodes, dtype=np.uint32)[:, local].reshape(-1)
    n_cells = elem_nodes.shape[0] * p ** dim
    offsets = (np.arange(1, n_cells + 1, dtype=np.uint64) * 2 ** dim).astype(np.uint32)
    types = np.full(n_cells, 12 if dim == 3 else 9, dtype=np.uint8)
    return conn, offsets, types


def group_payload(fields, inds, n_points):
    """fields: host (n_fields, ld); 1 row -> [n], 2 or 3 rows -> [n][3] with +0.0 in the third place of a group of 2"""
    if len(inds) == 1:
        return np.ascontiguousarray(fields[inds[0], :n_points], dtype="<f8")
    out = np.zeros((n_points, 3), dtype="<f8")
    for c, i in enumerate(inds):
        out[:, c] = fields[i, :n_points]
    return out


def n_components(inds):
    return 1 if len(inds) == 1 else 3


def active_arrays(groups):
    """` Scalars="first 1-component group" Vectors="first 3-component group"`, Scalars first; the same rule in both files"""
    scalar = next((name for name, inds in groups if len(inds) == 1), None)
    vector = next((name for name, inds in groups if len(inds) != 1), None)
    return (f' Scalars="{scalar}"' if scalar is not None else "") + (f' Vectors="{vector}"' if vector is not None else "")


def vtu_name(file_name, rank):
    return os.path.splitext(file_name)[0] + f"_{rank}.vtu"


def pvtu_name(file_name):
    return os.path.splitext(file_name)[0] + ".pvtu"


def vtu_header(n_points, n_cells, mesh_encoded_lens, groups):
    s = ('<?xml version="1.0"?>\n<VTKFile type="UnstructuredGrid" version="1.0" byte_order="LittleEndian" header_type="UInt64">\n'
         '<UnstructuredGrid>\n')
    s += f'<Piece NumberOfPoints="{n_points}" NumberOfCells="{n_cells}">\n'
    offset = 0

    def array(kind, name, nc, size):
        nonlocal offset
        text = f'  <DataArray type="{kind}" Name="{name}" NumberOfComponents="{nc}" format="appended" offset="{offset}">\n  </DataArray>\n'
        offset += size
        return text

    s += "<Points>\n" + array("Float64", "Position", 3, mesh_encoded_lens[0]) + "</Points>\n<Cells>\n"
    s += array("UInt32", "connectivity", 1, mesh_encoded_lens[1]) + array("UInt32", "offsets", 1, mesh_encoded_lens[2])
    s += array("UInt8", "types", 1, mesh_encoded_lens[3]) + "</Cells>\n"
    s += "<PointData" + active_arrays(groups) + ">\n"
    for name, inds in groups:
        s += array("Float64", name, n_components(inds), encoded_len(8 * n_points * n_components(inds)))
    s += '</PointData>\n<CellData>\n</CellData>\n</Piece>\n</UnstructuredGrid>\n<AppendedData encoding="base64">\n  _'
    return s.encode()


def vtu_bytes(part, groups, fields, coords=None):
    """the whole .vtu of a partition (anything with dim, order, elem_nodes, n_local_nodes, node_coords()); groups: [(name, [rows])];
    fields: host (n_fields, ld).  coords: the [n, 3] coordinates to write instead of part.node_coords()"""
    n_points = part.n_local_nodes
    coords = part.node_coords() if coords is None else coords
    conn, offsets, types = topology(part.elem_nodes, part.dim, part.order)
    sections = [encoded(np.ascontiguousarray(coords, dtype="<f8").tobytes()), encoded(conn.tobytes()), encoded(offsets.tobytes()),
                encoded(types.tobytes())]
    body = b"".join(sections)
    for _, inds in groups:
        body += encoded(group_payload(fields, inds, n_points).tobytes())
    head = vtu_header(n_points, len(types), [len(s) for s in sections], groups)
    return head + body + b"\n</AppendedData>\n</VTKFile>"


def pvtu_bytes(file_name, n_ranks, groups):
    s = ('<?xml version="1.0"?>\n<VTKFile type="PUnstructuredGrid" version="1.0" byte_order="LittleEndian">\n'
         '<PUnstructuredGrid GhostLevel="0">\n<PPoints>\n  <PDataArray type="Float64" Name="Position" NumberOfComponents="3"/>\n'
         '</PPoints>\n<PCells>\n  <PDataArray type="UInt32" Name="connectivity" NumberOfComponents="1"/>\n'
         '  <PDataArray type="UInt32" Name="offsets" NumberOfComponents="1"/>\n'
         '  <PDataArray type="UInt8" Name="types" NumberOfComponents="1"/>\n</PCells>\n<PPointData')
    s += active_arrays(groups) + ">\n"
    for name, inds in groups:
        s += f'  <PDataArray type="Float64" Name="{name}" NumberOfComponents="{n_components(inds)}"/>\n'
    s += "</PPointData>\n<PCellData>\n</PCellData>\n"
    stem = os.path.splitext(os.path.basename(file_name))[0]
    for r in range(n_ranks):
        s += f'<Piece Source="{stem}_{r}.vtu"/>\n'
    return (s + "</PUnstructuredGrid>\n</VTKFile>").encode()


def position_span(n_points):
    """(first byte, byte count) of the Position array's text inside the appended block"""
    return 0, encoded_len(24 * n_points)
