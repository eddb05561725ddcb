"""The ParaView export (l3ster_amd.vtk) measured: the encoder against a device copy, one export against the host route, the creation
of an exporter, and the chunk size.

    python tools/bench_vtk.py [--out profiles/vtk.jsonl] [--dirs /dev/shm,.] [--reps 5] [--chunks-mib 4,16,64,256]

One process, one untimed round first, the legs of a comparison alternate inside each repetition, medians.  Meshes: 32^3 hexes of order
4 and 64^2 quads of order 4; one scalar and one 3-row group.  One JSON line per (mesh, leg):
  (a) encode       l3k_vtk_encode on the payload of the 3-row group at 4, 8 and 16 text bytes per lane (L3K_VTK_STORE_BYTES), HIP
                   events around launches that walk over up to 8 distinct sets of buffers (600 MB in all on the hex mesh: past the
                   256 MiB last-level cache; sets_bytes in the line); effective bandwidth = (bytes read + bytes written) / time,
                   beside a device-to-device copy of the same total bytes (half read, half written) timed the same way
  (b) export       PvtuExporter.export_solution per target directory, beside the host route on the same data: the D2H copy of the
                   field rows, numpy interleave, base64.b64encode, and the write of the SAME file (mesh text cached, as the exporter's)
  (b') stages      what the export's three stages cost on their own for the text of the field arrays: encode (events), the pinned
                   D2H copy of the text (events), the write of that many bytes to the target (host clock)
  (c) create       PvtuExporter(mesh), host clock around the synchronous call
  (d) chunk        the export at each --chunks-mib
"""
import argparse
import base64
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GROUPS = [("T", [0]), ("velocity", [1, 2, 3])]


def median(v):
    return float(np.median(v))


def host_clock(f):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def event_seconds(f, launches=10):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / launches


def definition(path):
    from l3ster_amd import vtk
    d = vtk.ExportDefinition(path)
    for name, inds in GROUPS:
        d.define_field(name, inds)
    return d


def host_route(path, fields, n, head, mesh_text):
    """what a user of the parent commit had: the rows to the host, interleave and encode there, write"""
    rows = fields[:, :n].cpu().numpy()
    with open(path, "wb") as f:
        f.write(head)
        f.write(mesh_text)
        for _, inds in GROUPS:
            payload = rows[inds[0]] if len(inds) == 1 else np.ascontiguousarray(rows[inds].T)
            f.write(base64.b64encode(struct.pack("<Q", payload.nbytes) + payload.tobytes()))
        f.write(b"\n</AppendedData>\n</VTKFile>")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vtk.jsonl"))
    ap.add_argument("--dirs", default="/dev/shm,.")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunks-mib", default="4,16,64,256")
    ap.add_argument("--meshes", default="hex,quad")
    a = ap.parse_args()
    import torch
    from l3ster_amd import capi, system, vtk
    torch.cuda.set_device(0)
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    lib = capi.load()
    with open(a.out, "w") as out:
        def emit(line):
            line.update(device=torch.cuda.get_device_name(0), reps=a.reps)
            out.write(json.dumps(line) + "\n")
            out.flush()
            print(json.dumps(line), flush=True)

        for kind in a.meshes.split(","):
            part = system.CubePartition(32, 4) if kind == "hex" else system.SquarePartition(64, 4)
            tag = dict(mesh="32^3 hexes" if kind == "hex" else "64^2 quads", order=4, n_points=part.n_local_nodes)
            n = part.n_local_nodes
            dmesh = system.DeviceMesh(ctx, part, 1)
            fields = torch.randn((4, n), dtype=torch.float64, device="cuda")
            # ---- (c) creation
            t_create = [host_clock(lambda: vtk.PvtuExporter(dmesh)) for _ in range(a.reps + 1)][1:]
            exporter = vtk.PvtuExporter(dmesh)
            info = exporter.info()
            emit(dict(tag, leg="create", seconds=median(t_create), n_cells=info["n_cells"], mesh_text_bytes=sum(info["encoded_bytes"]),
                      chunk_bytes=info["chunk_bytes"]))
            # ---- (a) the encoder alone on the 3-component payload
            payload = fields[1:4].T.contiguous()
            n_bytes = payload.numel() * 8
            text = torch.empty(4 * ((8 + n_bytes + 2) // 3), dtype=torch.uint8, device="cuda")
            moved = n_bytes + text.numel()
            # the launches of a timing walk over `sets` distinct buffers, 600 MB in all where 8 sets reach that: past the 256 MiB
            # last-level cache, so that the large case is an HBM figure (the small case stays cache-resident: sets_bytes says which)
            sets = max(1, min(8, -(-600_000_000 // moved)))
            payloads = [payload] + [payload.clone() for _ in range(sets - 1)]
            texts = [text] + [torch.empty_like(text) for _ in range(sets - 1)]
            srcs = [torch.empty(moved // 2, dtype=torch.uint8, device="cuda") for _ in range(sets)]
            dsts = [torch.empty_like(s) for s in srcs]
            turn = [0]

            def encode_next():
                k = turn[0] = (turn[0] + 1) % sets
                capi.check(lib.l3k_vtk_encode(ctx._h, payloads[k].data_ptr(), n_bytes, texts[k].data_ptr(), text.numel()))

            def copy_next():
                k = turn[0] = (turn[0] + 1) % sets
                dsts[k].copy_(srcs[k])

            times = {w: [] for w in (4, 8, 16, "copy")}
            for rep in range(a.reps + 1):
                for w in (4, 8, 16):
                    os.environ["L3K_VTK_STORE_BYTES"] = str(w)
                    times[w].append(event_seconds(encode_next, 2 * sets))
                times["copy"].append(event_seconds(copy_next, 2 * sets))
            del payloads, texts, srcs, dsts
            os.environ.pop("L3K_VTK_STORE_BYTES")
            t_copy = median(times["copy"][1:])
            for w in (4, 8, 16):
                t = median(times[w][1:])
                emit(dict(tag, leg="encode", store_bytes=w, payload_bytes=n_bytes, text_bytes=text.numel(), sets_bytes=sets * moved, seconds=t,
                          bytes_per_s=moved / t, d2d_copy_seconds=t_copy, d2d_copy_bytes_per_s=moved / t_copy, fraction_of_copy=t_copy / t))
            # ---- (b') the stages of an export on their own: encode both arrays, copy their text, write it
            field_text = sum(4 * ((8 + 8 * n * (1 if len(i) == 1 else 3) + 2) // 3) for _, i in GROUPS)
            t_encode = median(times[info["store_bytes"]][1:]) * field_text / text.numel()
            pinned = torch.empty(field_text, dtype=torch.uint8, pin_memory=True)
            dev_text = torch.empty(field_text, dtype=torch.uint8, device="cuda")
            t_d2h = median([event_seconds(lambda: pinned.copy_(dev_text, non_blocking=True), 3) for _ in range(a.reps + 1)][1:])
            for d in a.dirs.split(","):
                work = os.path.join(os.path.abspath(d), "bench_vtk_tmp")
                os.makedirs(work, exist_ok=True)
                blob = pinned.numpy().tobytes()

                def write_blob():
                    with open(os.path.join(work, "blob"), "wb") as f:
                        f.write(blob)

                t_write = median([host_clock(write_blob) for _ in range(a.reps + 1)][1:])
                emit(dict(tag, leg="stages", dir=d, field_text_bytes=field_text, encode_seconds=t_encode, d2h_copy_seconds=t_d2h,
                          write_seconds=t_write))
                # ---- (b) one export against the host route, alternating
                head = vtk.vtu_header_text(definition("x"), n, info["n_cells"], info["encoded_bytes"])
                exporter.export_solution(definition(os.path.join(work, "dev.pvtu")), fields)
                whole = open(os.path.join(work, "dev_0.vtu"), "rb").read()
                mesh_text = whole[len(head):len(head) + sum(info["encoded_bytes"])]
                t_dev, t_host = [], []
                for rep in range(a.reps + 1):
                    t_dev.append(host_clock(lambda: exporter.export_solution(definition(os.path.join(work, "dev.pvtu")), fields)))
                    t_host.append(host_clock(lambda: host_route(os.path.join(work, "host_0.vtu"), fields, n, head, mesh_text)))
                same = open(os.path.join(work, "host_0.vtu"), "rb").read() == whole
                emit(dict(tag, leg="export", dir=d, file_bytes=len(whole), seconds=median(t_dev[1:]), host_route_seconds=median(t_host[1:]),
                          speedup=median(t_host[1:]) / median(t_dev[1:]), files_identical=same, chunk_bytes=info["chunk_bytes"]))
                # ---- (d) the chunk size
                for mib in (int(s) for s in a.chunks_mib.split(",")):
                    ex = vtk.PvtuExporter(dmesh, chunk_bytes=mib << 20)
                    t = [host_clock(lambda: ex.export_solution(definition(os.path.join(work, "chunk.pvtu")), fields)) for _ in range(a.reps + 1)]
                    emit(dict(tag, leg="chunk", dir=d, chunk_mib=mib, chunk_bytes=ex.info()["chunk_bytes"], seconds=median(t[1:])))
                    del ex
                for name in os.listdir(work):
                    os.remove(os.path.join(work, name))
                os.rmdir(work)


if __name__ == "__main__":
    main()
