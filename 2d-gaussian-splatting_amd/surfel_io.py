"""On-disk formats of the reference without third-party readers: `point_cloud.ply` as
scene/gaussian_model.py:193-207 writes it through plyfile (binary little-endian, one `vertex` element, float32
properties x,y,z,nx,ny,nz,f_dc_*,f_rest_*,opacity,scale_*,rot_*) and as :214-255 reads it back.  numpy only.
"""
import os

import numpy as np

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def write_ply(path, names, columns):
    """columns: [P, len(names)] float32 -> binary_little_endian PLY with one float property per name."""
    columns = np.ascontiguousarray(columns, dtype="<f4")
    if columns.ndim != 2 or columns.shape[1] != len(names):
        raise ValueError("columns must be [P, %d]" % len(names))
    header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % columns.shape[0]]
    header += ["property float %s" % n for n in names] + ["end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(columns.tobytes())


def write_ply_records(path, rec):
    """rec: 1-D structured array of scalar little-endian fields -> binary_little_endian PLY with one `vertex` property per field, each of
    its own type (e.g. the float x y z nx ny nz + uchar red green blue of the reference's points3D.ply)."""
    names = {"i1": "char", "u1": "uchar", "i2": "short", "u2": "ushort", "i4": "int", "u4": "uint", "f4": "float", "f8": "double"}
    rec = np.ascontiguousarray(rec)
    header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % rec.shape[0]]
    for n in rec.dtype.names:
        t = rec.dtype[n]
        if t.shape or t.byteorder == ">" or t.str[1:] not in names:
            raise ValueError("field %s: unsupported type %s" % (n, t))
        header.append("property %s %s" % (names[t.str[1:]], n))
    with open(path, "wb") as f:
        f.write(("\n".join(header + ["end_header"]) + "\n").encode("ascii"))
        f.write(rec.tobytes())


def read_ply(path):
    """Returns {property name: 1-D numpy array} of the first element (`vertex`).  Handles binary little/big endian and
    ascii; list properties are not supported (the reference's point clouds have none)."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("%s is not a PLY file" % path)
        fmt, count, props, in_first, n_elements = None, None, [], False, 0
        while True:
            line = f.readline()
            if not line:
                raise ValueError("%s: truncated PLY header" % path)
            tok = line.decode("ascii").split()
            if not tok or tok[0] == "comment" or tok[0] == "obj_info":
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                n_elements += 1
                in_first = n_elements == 1
                if in_first:
                    count = int(tok[2])
            elif tok[0] == "property" and in_first:
                if tok[1] == "list":
                    raise ValueError("%s: list properties are not supported" % path)
                props.append((tok[2], _PLY_TYPES[tok[1]]))
            elif tok[0] == "end_header":
                break
        if fmt is None or count is None:
            raise ValueError("%s: PLY header lacks format / element" % path)
        if fmt == "ascii":
            data = np.loadtxt(f, max_rows=count, ndmin=2)
            return {n: data[:, i].astype(t) for i, (n, t) in enumerate(props)}
        order = "<" if fmt == "binary_little_endian" else ">"
        dt = np.dtype([(n, order + t) for n, t in props])
        rec = np.frombuffer(f.read(count * dt.itemsize), dtype=dt, count=count)
        return {n: np.ascontiguousarray(rec[n]) for n, _ in props}


# ------------------------------------------------------------------------------------------------ triangle meshes and cameras
def write_triangle_mesh(path, mesh):
    """Binary little-endian PLY of a mesh with .vertices [V,3], .vertex_colors [V,3] (0..1) and .triangles [F,3] (numpy arrays or
    tensors): float x,y,z, uchar red,green,blue per vertex and `list uchar int vertex_indices` per face."""
    def host(x):
        return np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x)
    v = host(mesh.vertices).astype("<f4").reshape(-1, 3)
    c = host(mesh.vertex_colors).reshape(-1, 3)
    f = host(mesh.triangles).astype("<i4").reshape(-1, 3)
    vrec = np.empty(v.shape[0], dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])
    vrec["xyz"] = v
    vrec["rgb"] = np.round(np.clip(c, 0.0, 1.0) * 255.0).astype(np.uint8) if c.size else c.astype(np.uint8)
    frec = np.empty(f.shape[0], dtype=[("n", "u1"), ("idx", "<i4", 3)])
    frec["n"] = 3
    frec["idx"] = f
    header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % v.shape[0], "property float x", "property float y",
              "property float z", "property uchar red", "property uchar green", "property uchar blue", "element face %d" % f.shape[0],
              "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())


def read_triangle_mesh(path):
    """(vertices [V,3] float32, triangles [F,3] int32, vertex_colors [V,3] float32 in 0..1) of a binary little-endian PLY with
    float x,y,z (+ optional uchar red,green,blue) vertices and triangle faces (`list uchar int|uint vertex_indices`)."""
    with open(path, "rb") as fh:
        if fh.readline().strip() != b"ply":
            raise ValueError("%s is not a PLY file" % path)
        elements, cur = [], None
        while True:
            line = fh.readline()
            if not line:
                raise ValueError("%s: truncated PLY header" % path)
            tok = line.decode("ascii").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "format" and tok[1] != "binary_little_endian":
                raise ValueError("%s: only binary_little_endian meshes are supported" % path)
            if tok[0] == "element":
                cur = [tok[1], int(tok[2]), []]
                elements.append(cur)
            elif tok[0] == "property":
                cur[2].append(tuple(tok[1:]))
            elif tok[0] == "end_header":
                break
        verts = tris = cols = None
        for name, count, props in elements:
            if name == "vertex":
                dt = np.dtype([(p[1], "<" + _PLY_TYPES[p[0]]) for p in props])
                rec = np.frombuffer(fh.read(count * dt.itemsize), dtype=dt, count=count)
                verts = np.stack([rec["x"], rec["y"], rec["z"]], 1).astype(np.float32)
                if "red" in dt.names:
                    cols = np.stack([rec["red"], rec["green"], rec["blue"]], 1).astype(np.float32) / 255.0
                else:
                    cols = np.zeros((count, 3), np.float32)
            elif name == "face":
                if len(props) != 1 or props[0][0] != "list":
                    raise ValueError("%s: faces must hold one list property" % path)
                dt = np.dtype([("n", _PLY_TYPES[props[0][1]]), ("idx", "<" + _PLY_TYPES[props[0][2]], 3)])
                rec = np.frombuffer(fh.read(count * dt.itemsize), dtype=dt, count=count)
                if count and np.any(rec["n"] != 3):
                    raise ValueError("%s: only triangle faces are supported" % path)
                tris = rec["idx"].astype(np.int32).reshape(-1, 3)
            else:
                raise ValueError("%s: unexpected element %s" % (path, name))
    if tris is None:
        tris = np.zeros((0, 3), np.int32)
    return verts, tris, cols


def ply_stem(path):
    """MESH of MESH.ply: what the mesh tools append _smoothed.ply, _cull.ply, ... to; any other path as it is"""
    return path[:-4] if path.endswith(".ply") else path


def write_obj(path, vertices, triangles, vt=None, texture=None):
    """Wavefront OBJ of a mesh (numpy arrays or tensors): `v x y z` per vertex, `f a b c` per triangle (1-based).  vt [F, 3, 2]: three
    texture coordinates per triangle in OBJ's convention (the origin at the image's lower left corner), written as 3 F `vt u v` lines
    and `f a/ta b/tb c/tc`.  texture: the image's file name; a material library beside the OBJ (the same name with .mtl) names it."""
    def host(x):
        return np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x)
    v = host(vertices).astype(np.float32).reshape(-1, 3)
    f = host(triangles).astype(np.int64).reshape(-1, 3)
    lines = []
    if texture is not None:
        mtl = os.path.splitext(os.path.basename(path))[0] + ".mtl"
        with open(os.path.join(os.path.dirname(path), mtl), "w") as fh:
            fh.write("newmtl atlas\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd %s\n" % texture)
        lines += ["mtllib %s" % mtl, "usemtl atlas"]
    lines += ["v %.9g %.9g %.9g" % tuple(p) for p in v.tolist()]
    if vt is None:
        lines += ["f %d %d %d" % (a + 1, b + 1, c + 1) for a, b, c in f.tolist()]
    else:
        t = host(vt).astype(np.float32).reshape(-1, 2)
        if len(t) != 3 * len(f):
            raise ValueError("write_obj: %d texture coordinates for %d triangles" % (len(t), len(f)))
        lines += ["vt %.9g %.9g" % tuple(q) for q in t.tolist()]
        lines += ["f %d/%d %d/%d %d/%d" % (a + 1, 3 * k + 1, b + 1, 3 * k + 2, c + 1, 3 * k + 3) for k, (a, b, c) in enumerate(f.tolist())]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def read_obj(path):
    """(vertices [V, 3] float32, triangles [F, 3] int32, vt [F, 3, 2] float32 or None, texture file name or None) of an OBJ that write_obj
    wrote, or of a plain `v` / `f` file: triangle faces only, `f a b c`, `f a/ta ...` or `f a/ta/na ...` with positive or negative
    indices; map_Kd of the first material library names the texture."""
    v, vt, f, ft, texture = [], [], [], [], None
    with open(path) as fh:
        for line in fh:
            tok = line.split()
            if not tok or tok[0].startswith("#"):
                continue
            if tok[0] == "v":
                v.append([float(x) for x in tok[1:4]])
            elif tok[0] == "vt":
                vt.append([float(x) for x in tok[1:3]])
            elif tok[0] == "f":
                if len(tok) != 4:
                    raise ValueError("%s: only triangle faces are supported" % path)
                parts = [x.split("/") for x in tok[1:]]
                f.append([int(x[0]) for x in parts])
                if all(len(x) > 1 and x[1] for x in parts):
                    ft.append([int(x[1]) for x in parts])
            elif tok[0] == "mtllib" and texture is None:
                mtl = os.path.join(os.path.dirname(path), line.split(None, 1)[1].strip())
                if os.path.exists(mtl):
                    for ml in open(mtl):
                        if ml.split() and ml.split()[0] == "map_Kd":
                            texture = ml.split(None, 1)[1].strip()
                            break
    verts = np.asarray(v, np.float32).reshape(-1, 3)
    tris = np.asarray(f, np.int64).reshape(-1, 3)
    tris = np.where(tris < 0, tris + len(verts), tris - 1).astype(np.int32)
    uv = None
    if ft:
        if len(ft) != len(f):
            raise ValueError("%s: some faces carry texture coordinates and some do not" % path)
        idx = np.asarray(ft, np.int64)
        idx = np.where(idx < 0, idx + len(vt), idx - 1)
        uv = np.asarray(vt, np.float32).reshape(-1, 2)[idx]
    return verts, tris, uv, texture


def read_cameras_json(path, device="cuda"):
    """surfel_render.Camera list from the reference's cameras.json (utils/camera_utils.py:64-84 writes it: `position` and `rotation` are
    the camera-to-world translation and rotation, fx / fy in pixels).  The cameras carry a black placeholder image of their size."""
    import json
    import torch
    from surfel_render import Camera
    cams = []
    for e in json.load(open(path)):
        R = np.asarray(e["rotation"], np.float64)           # C2W rotation = the reference's Camera.R
        T = -R.T @ np.asarray(e["position"], np.float64)    # W2C translation
        W, H = int(e["width"]), int(e["height"])
        fovx, fovy = 2 * np.arctan(W / (2 * float(e["fx"]))), 2 * np.arctan(H / (2 * float(e["fy"])))
        cams.append(Camera(colmap_id=e["id"], R=R, T=T, FoVx=fovx, FoVy=fovy, image=torch.zeros(3, H, W), image_name=e.get("img_name", ""),
                           uid=e["id"], data_device=device))
    return cams
