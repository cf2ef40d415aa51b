"""NumPy restatement of what a brick optimiser starts from (include/knerf.h "Optimising a brick field as it is"), written from the
specification and not from the package; plain loops, meant for the small lattices of the tests: the train-brick set, the flag of
every stored record and the map from a row to its lattice point.  Built from tests/baked_train_reference.py (support_cells,
slot_points, sigma_trainable) and tests/baked_bricks_reference.py (the brick format).

Gradients and Adam are NOT restated here.  The reference of a brick optimiser over a brick field F is tests/baked_train_reference.py
on the dense arrays of F, dense_from_bricks(F): a point of an absent brick holds sigma 0 and zero coefficients there.
"""
import numpy as np

from tests import baked_bricks_reference as B
from tests import baked_train_reference as T

FLAG_SLOT, FLAG_SIGMA = 1, 2


def train_bricks(sigma, b, dilation=0):
    """(support bool cells, brick_of int32 [Bx,By,Bz], n): the support of the dense optimiser and the bricks that hold a corner of one
    of its cells, numbered in ascending C order like the stored bricks of a brick field"""
    support = T.support_cells(sigma, dilation)
    brick_of, n = B.brick_table(support, sigma.shape, b)
    return support, brick_of, n


def row_points(brick_of, resolution, b):
    """int64 [n b^3]: the linear lattice index of every row (row = slot b^3 + place), -1 for a place past the lattice"""
    R = tuple(int(r) for r in resolution)
    n = int((brick_of >= 0).sum())
    out = np.full((n, b, b, b), -1, dtype=np.int64)
    for (bx, by, bz), slot in np.ndenumerate(brick_of):
        if slot < 0:
            continue
        for i in range(b):
            for j in range(b):
                for k in range(b):
                    x, y, z = bx * b + i, by * b + j, bz * b + k
                    if x < R[0] and y < R[1] and z < R[2]:
                        out[slot, i, j, k] = (x * R[1] + y) * R[2] + z
    return out.reshape(-1)


def flags(support, brick_of, b):
    """uint8 [n b^3]: bit 0 = the row's point is a corner of a support cell, bit 1 = its sigma is trainable; 0 past the lattice"""
    slots, train = T.slot_points(support), T.sigma_trainable(support)
    at = row_points(brick_of, slots.shape, b)
    out = np.zeros(at.shape, dtype=np.uint8)
    inside = at >= 0
    out[inside] = slots.reshape(-1)[at[inside]] * FLAG_SLOT + train.reshape(-1)[at[inside]] * FLAG_SIGMA
    return out


def master_rows(sigma, coefficients, support, brick_of, b):
    """float32 [n b^3, 1 + 3 K]: (sigma where it is trainable else 0, the fp16 coefficients widened) of every row's point in the DENSE
    arrays of the field; zero rows past the lattice"""
    K = coefficients.shape[3]
    at = row_points(brick_of, sigma.shape, b)
    train = T.sigma_trainable(support).reshape(-1)
    out = np.zeros((at.size, 1 + 3 * K), dtype=np.float32)
    inside = at >= 0
    p = at[inside]
    out[inside, 0] = sigma.reshape(-1)[p].astype(np.float32) * train[p]
    out[inside, 1:] = coefficients.reshape(-1, 3 * K)[p].astype(np.float16).astype(np.float32)
    return out


def dense_arrays(brick_records, brick_of, resolution, b, degree):
    """(sigma fp32 [Rx,Ry,Rz], coefficients fp16 [Rx,Ry,Rz,K,3]) of a brick field: what the reference optimiser is run on"""
    R = tuple(int(r) for r in resolution)
    K = (degree + 1) ** 2
    rec = B.dense_from_bricks(brick_records, brick_of, R, b)
    sg = np.ascontiguousarray(rec[:, :4]).view(np.float32).reshape(R)
    co = np.ascontiguousarray(rec[:, 4:4 + 6 * K]).view(np.float16).reshape(R + (K, 3))
    return sg, co
