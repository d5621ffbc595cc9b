"""What the GPU tests of the mesh tools share: host arrays and meshes put on the device."""
import numpy as np
import torch


def dev():
    return torch.device("cuda:0")


def to_device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def mesh(v, t, c=None):
    """surfel_mesh.TriangleMesh of float32 vertices, int32 triangles and float32 colours (None: a mesh without colours)"""
    from surfel_mesh import TriangleMesh
    return TriangleMesh(to_device(np.asarray(v, np.float32)), to_device(np.asarray(t, np.int32)),
                        to_device(np.asarray(c, np.float32)) if c is not None else None)
