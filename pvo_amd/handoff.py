"""On-disk hand-off to the video-panoptic-segmentation half of PVO (out of scope here): per image pair one
`.npy` with the full optical flow and one with the inverse depth, as evaluation_scripts/test_vo2.py:131-143
writes them (`<root>/full_flow/<id>.npy`, `<root>/depth/<id>.npy`, float32, written with numpy.save)."""
import os

import numpy as np
import torch
import torch.nn.functional as F


def _resize_bilinear(a, size_hw):
    """half-pixel-centre bilinear resize of an [H,W,C] array (what cv2.resize's default does, test_vo2.py:136)"""
    t = torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1)[None].float()
    return F.interpolate(t, size=size_hw, mode="bilinear", align_corners=False)[0].permute(1, 2, 0).numpy()


def save_flow_depth(root, img_id, full_flow, disp, valid=None, resize_hw=None):
    """full_flow [H,W,2] (pixels, image resolution), disp [H,W] inverse depth, valid [H,W,1] optional mask.
    Returns the two paths written."""
    flow = full_flow.detach().cpu().numpy() if isinstance(full_flow, torch.Tensor) else np.asarray(full_flow)
    flow = flow.astype(np.float32)
    if valid is not None:
        flow = flow * (valid.detach().cpu().numpy() if isinstance(valid, torch.Tensor) else np.asarray(valid))
    if resize_hw is not None:
        flow = _resize_bilinear(flow, resize_hw)
    depth = (disp.detach().cpu().numpy() if isinstance(disp, torch.Tensor) else np.asarray(disp)).astype(np.float32)
    paths = []
    for sub, arr in (("full_flow", flow), ("depth", depth)):
        d = os.path.join(root, sub)
        os.makedirs(d, exist_ok=True)
        paths.append(os.path.join(d, img_id + ".npy"))
        np.save(paths[-1], arr)
    return paths


def write_kitti_trajectory(path, traj):
    """[N,7] (t, q xyzw) camera-to-world poses -> KITTI format, 12 numbers per line (the file test_vo.py:150-159
    writes through evo's write_kitti_poses_file)."""
    from .geom.se3 import SE3
    T = SE3(torch.as_tensor(np.asarray(traj), dtype=torch.float64)).matrix().numpy()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        for m in T:
            f.write(" ".join("%.9e" % v for v in m[:3].reshape(-1)) + "\n")


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def write_ply(path, xyz, rgb=None, label=None, sigma=None):
    """a point cloud as binary little-endian PLY: x y z float, then red green blue uchar (rgb [n,3] or [n,4], the first three columns;
    omitted when None), then an int label (omitted when None), then a float sigma - the point's standard deviation of the inverse
    depth (omitted when None: the file is then byte for byte what it was without the argument).  numpy only; returns the number of
    points written."""
    xyz = _host(xyz)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    props = ["property float x", "property float y", "property float z"]
    if rgb is not None:
        rgb = _host(rgb)
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        props += ["property uchar red", "property uchar green", "property uchar blue"]
    if label is not None:
        label = _host(label)
        fields.append(("label", "<i4"))
        props.append("property int label")
    if sigma is not None:
        sigma = _host(sigma)
        fields.append(("sigma", "<f4"))
        props.append("property float sigma")
    n = int(xyz.shape[0])
    rec = np.zeros(n, dtype=np.dtype(fields))
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if rgb is not None:
        rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    if label is not None:
        rec["label"] = label
    if sigma is not None:
        rec["sigma"] = sigma
    header = "\n".join(["ply", "format binary_little_endian 1.0", "element vertex %d" % n] + props + ["end_header"]) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())
    return n


def write_ply_mesh(path, verts, faces, rgb=None, normals=None, label=None):
    """a triangle mesh as binary little-endian PLY: per vertex x y z float, then nx ny nz float (omitted when normals is None), then
    red green blue uchar (rgb [n,3] or [n,4], the first three columns; omitted when None), then an int label (the vertex's segment
    id; omitted when None: the file is then byte for byte what it was without the argument); per face `property list uchar int
    vertex_indices`: the byte 3 and three int32 indices.  numpy only; returns (vertices, faces) written."""
    verts, faces = _host(verts), _host(faces)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    props = ["property float x", "property float y", "property float z"]
    if normals is not None:
        normals = _host(normals)
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        props += ["property float nx", "property float ny", "property float nz"]
    if rgb is not None:
        rgb = _host(rgb)
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        props += ["property uchar red", "property uchar green", "property uchar blue"]
    if label is not None:
        label = _host(label)
        fields.append(("label", "<i4"))
        props.append("property int label")
    n, m = int(verts.shape[0]), int(faces.shape[0])
    rec = np.zeros(n, dtype=np.dtype(fields))
    rec["x"], rec["y"], rec["z"] = verts[:, 0], verts[:, 1], verts[:, 2]
    if normals is not None:
        rec["nx"], rec["ny"], rec["nz"] = normals[:, 0], normals[:, 1], normals[:, 2]
    if rgb is not None:
        rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    if label is not None:
        rec["label"] = label.reshape(n)
    tri = np.zeros(m, dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    tri["n"], tri["v"] = 3, faces.reshape(m, 3)
    header = "\n".join(["ply", "format binary_little_endian 1.0", "element vertex %d" % n] + props +
                       ["element face %d" % m, "property list uchar int vertex_indices", "end_header"]) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())
        f.write(tri.tobytes())
    return n, m


_PLY_TYPES = {"float": "<f4", "uchar": "u1", "int": "<i4"}


def read_ply_mesh(path):
    """a file of write_ply_mesh back as numpy: dict verts f32 [n,3], faces int32 [m,3], and normals f32 [n,3] / rgb uint8 [n,3] /
    label int32 [n] where the file has them"""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    n = int([l for l in lines if l.startswith("element vertex")][0].split()[2])
    m = int([l for l in lines if l.startswith("element face")][0].split()[2])
    fields = [(l.split()[2], _PLY_TYPES[l.split()[1]]) for l in lines if l.startswith("property") and not l.startswith("property list")]
    dt = np.dtype(fields)
    rec = np.frombuffer(data, dt, n, end)
    tri = np.frombuffer(data, np.dtype([("n", "u1"), ("v", "<i4", (3,))]), m, end + n * dt.itemsize)
    out = {"verts": np.stack([rec["x"], rec["y"], rec["z"]], 1), "faces": tri["v"].copy()}
    names = [k for k, _ in fields]
    if "nx" in names:
        out["normals"] = np.stack([rec["nx"], rec["ny"], rec["nz"]], 1)
    if "red" in names:
        out["rgb"] = np.stack([rec["red"], rec["green"], rec["blue"]], 1)
    if "label" in names:
        out["label"] = rec["label"].copy()
    return out


def split_mesh_by_label(verts, faces, vlabel):
    """a labelled mesh cut into one mesh per segment id: {id: (verts [n_id,3], faces [m_id,3])}.  A face goes to the label that at
    least two of its vertices share, else to its first vertex's label; a part holds the vertices its faces use, in their old order,
    and its faces name them by their new indices.  numpy only."""
    verts, faces, vlabel = _host(verts), _host(faces).reshape(-1, 3), _host(vlabel).reshape(-1)
    l = vlabel[faces] if len(faces) else np.zeros((0, 3), vlabel.dtype)
    owner = np.where(l[:, 1] == l[:, 2], l[:, 1], l[:, 0])          # (0 == 1 or 0 == 2: the first's; 1 == 2: theirs; else the first's)
    out = {}
    for i in np.unique(owner):
        f = faces[owner == i]
        used = np.unique(f)
        remap = np.full(len(verts), -1, np.int64)
        remap[used] = np.arange(len(used))
        out[int(i)] = (verts[used], remap[f].astype(np.int32))
    return out


def save_reconstruction(root, video):
    """upstream DROID-SLAM's reconstruction folder (demo.py save_reconstruction): tstamps / disps / poses / intrinsics as .npy of
    the stored keyframes, and images when the video keeps them.  disps are the full-resolution maps where the video maintains them
    (tracking with args.upsample, as upstream saves disps_up), else the 1/8 maps; intrinsics are the stored ones, for the 1/8 maps.
    Returns the paths written."""
    n = video.counter
    os.makedirs(root, exist_ok=True)
    items = [("tstamps", video.tstamp[:n]), ("disps", (video.disps if video.disps_up is None else video.disps_up)[:n]),
             ("poses", video.poses[:n]), ("intrinsics", video.intrinsics[:n])]
    if video.images is not None:
        items.append(("images", video.images[:n]))
    paths = []
    for name, t in items:
        paths.append(os.path.join(root, name + ".npy"))
        np.save(paths[-1], _host(t))
    return paths
