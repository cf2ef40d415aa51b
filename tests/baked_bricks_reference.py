"""NumPy restatement of the brick format of a baked field (include/knerf.h "The baked field as sparse bricks"), written from the
specification and not from the package; plain loops, meant for the small lattices of the tests.

The lattice [Rx][Ry][Rz] is cut into bricks of b^3 lattice points, b = 4 or 8.  Point (x, y, z) lies in brick (x // b, y // b, z // b) of
the brick grid B_a = ceil(R_a / b), at place ((x % b) b + (y % b)) b + (z % b).  A brick is stored iff it holds a touched point (a corner
of a cell whose occupancy bit is set); stored bricks are numbered in ascending C order of the brick index; brick_of holds the slot
or -1.  A stored brick is a verbatim copy of the dense records of all its points, places outside the lattice are zero records, a field
without an occupied cell has one all-zero brick 0 that no entry names.  Absent bricks read as zero records.
"""
import numpy as np


def touched_points(occupied):
    """bool [Rx,Ry,Rz]: the corners of the occupied cells (occupied: bool [Rx-1,Ry-1,Rz-1])"""
    occ = np.asarray(occupied, dtype=bool)
    t = np.zeros(tuple(c + 1 for c in occ.shape), dtype=bool)
    for x, y, z in np.argwhere(occ):
        t[x:x + 2, y:y + 2, z:z + 2] = True
    return t


def brick_grid(resolution, b):
    return tuple(-(-int(r) // b) for r in resolution)


def brick_table(occupied, resolution, b):
    """(brick_of int32 [Bx,By,Bz], n_bricks >= 1)"""
    assert b in (4, 8)
    touched = touched_points(occupied)
    assert touched.shape == tuple(resolution)
    B = brick_grid(resolution, b)
    brick_of = np.full(B, -1, dtype=np.int32)
    n = 0
    for bx in range(B[0]):
        for by in range(B[1]):
            for bz in range(B[2]):
                if touched[bx * b:(bx + 1) * b, by * b:(by + 1) * b, bz * b:(bz + 1) * b].any():
                    brick_of[bx, by, bz] = n
                    n += 1
    return brick_of, max(n, 1)


def bricks_from_dense(records, brick_of, n_bricks, resolution, b):
    """dense records uint8 [P, record bytes] -> uint8 [n_bricks, b^3, record bytes]"""
    R = tuple(int(r) for r in resolution)
    rec = np.asarray(records, dtype=np.uint8).reshape(R + (-1,))
    out = np.zeros((n_bricks, b, b, b, rec.shape[-1]), dtype=np.uint8)
    for (bx, by, bz), slot in np.ndenumerate(brick_of):
        if slot < 0:
            continue
        part = rec[bx * b:(bx + 1) * b, by * b:(by + 1) * b, bz * b:(bz + 1) * b]
        out[slot, :part.shape[0], :part.shape[1], :part.shape[2]] = part
    return out.reshape(n_bricks, b ** 3, -1)


def dense_from_bricks(brick_records, brick_of, resolution, b):
    """uint8 [n_bricks, b^3, record bytes] -> dense uint8 [P, record bytes]; zero records where the brick is absent"""
    R = tuple(int(r) for r in resolution)
    br = np.asarray(brick_records, dtype=np.uint8)
    br = br.reshape(br.shape[0], b, b, b, -1)
    out = np.zeros(R + (br.shape[-1],), dtype=np.uint8)
    for (bx, by, bz), slot in np.ndenumerate(brick_of):
        if slot < 0:
            continue
        part = out[bx * b:(bx + 1) * b, by * b:(by + 1) * b, bz * b:(bz + 1) * b]
        part[...] = br[slot, :part.shape[0], :part.shape[1], :part.shape[2]]
    return out.reshape(-1, br.shape[-1])


def lookup(brick_records, brick_of, b, x, y, z):
    """the record of lattice point (x, y, z) as the renderer reads it: through the table, zeros for an absent brick"""
    slot = int(brick_of[x // b, y // b, z // b])
    if slot < 0 or slot >= brick_records.shape[0]:
        return np.zeros(brick_records.shape[-1], dtype=np.uint8)
    return brick_records[slot, ((x % b) * b + (y % b)) * b + (z % b)]


def partial_edge_bricks(brick_of, resolution, b):
    """bool [Bx,By,Bz]: stored bricks that reach past the lattice on some axis"""
    B = brick_of.shape
    past = np.zeros(B, dtype=bool)
    for a in range(3):
        if resolution[a] % b:
            sl = [slice(None)] * 3
            sl[a] = B[a] - 1
            past[tuple(sl)] = True
    return past & (brick_of >= 0)
