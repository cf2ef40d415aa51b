"""NumPy restatement of growing a brick baked field (include/knerf.h "Growing a brick field as it is"), written from the specification
and not from the package; plain loops where there are any, meant for the small lattices of the tests.  Nothing is restated that another
reference already states: resampling is tests/baked_grow_reference.py on the dense arrays of the field cut into bricks again by
tests/baked_bricks_reference.py, the regulariser is tests/baked_grow_reference.py's with the rows of
tests/baked_bricks_train_reference.py as its slots, and what a prune builds is the train state of the finished field.
"""
import numpy as np

from tests import baked_bricks_reference as B
from tests import baked_bricks_train_reference as S
from tests import baked_grow_reference as G
from tests import baked_reference as R


def resample(brick_records, brick_of, res, b, res_new, degree, threshold=0.0, b_new=None):
    """A brick field on another lattice: bricks_from_dense(resample_mirror(dense_from_bricks(F))).  Returns (sigma fp32 [R'] after the
    threshold, occupied cells bool, brick_of', n_bricks', records' uint8 [n', b'^3, record bytes])."""
    b_new = b if b_new is None else b_new
    dense = B.dense_from_bricks(brick_records, brick_of, res, b)
    sigma, _, rec = G.resample(dense, tuple(res), tuple(res_new), degree, threshold, np.float32)
    occ = R.occupied_cells(sigma.reshape(res_new))
    of, n = B.brick_table(occ, tuple(res_new), b_new)
    return sigma.reshape(res_new), occ, of, n, B.bricks_from_dense(rec, of, n, tuple(res_new), b_new)


def slot_of_rows(brick_of, flags, res, b):
    """int64 [points]: the row of every lattice point whose record has flag bit 0, -1 elsewhere: the slot table under which
    tests/baked_grow_reference.py tv_value_and_grad, given the rows [n_bricks b^3, W] as its master, is the regulariser of a brick
    optimiser (rows that no entry names get a zero gradient there and never enter a difference)"""
    at = S.row_points(brick_of, res, b)
    out = np.full(int(np.prod(res)), -1, dtype=np.int64)
    rows = np.flatnonzero((at >= 0) & ((np.asarray(flags) & S.FLAG_SLOT) != 0))
    out[at[rows]] = rows
    return out


def tv_value_and_grad(master, brick_of, flags, res, b, w_sigma, w_sh, eps, dtype=np.float64):
    """tests/baked_grow_reference.py tv_value_and_grad over the rows of a brick optimiser: (R, grad [n_bricks b^3, W], (two sums))"""
    return G.tv_value_and_grad(master, slot_of_rows(brick_of, flags, res, b), tuple(res), w_sigma, w_sh, eps, dtype)


def carried_rows(old_brick_of, old_flags, new_brick_of, new_flags, res, b):
    """What a prune carries, row by row of the new train bricks: (old_row int64 [n_new b^3]: the old row of the same lattice point where
    the point has flag bit 0 before and after, else -1; sigma bool: that, and bit 1 before and after)"""
    old_at, new_at = S.row_points(old_brick_of, res, b), S.row_points(new_brick_of, res, b)
    row_of = {}
    for r, p in enumerate(old_at):
        if p >= 0 and old_flags[r] & S.FLAG_SLOT:
            row_of[int(p)] = r
    old_row = np.full(new_at.size, -1, dtype=np.int64)
    sigma = np.zeros(new_at.size, dtype=bool)
    for r, p in enumerate(new_at):
        if p >= 0 and new_flags[r] & S.FLAG_SLOT and int(p) in row_of:
            old_row[r] = row_of[int(p)]
            sigma[r] = bool(new_flags[r] & S.FLAG_SIGMA) and bool(old_flags[old_row[r]] & S.FLAG_SIGMA)
    return old_row, sigma


def train_state(sigma, coefficients, b, dilation):
    """(support, brick_of, n, flags, master fp32) a brick optimiser starts from on the dense arrays (sigma fp32, coefficients fp16): what
    grid_trainer(field) builds, and, with the arrays of finish(threshold), what prune(threshold) leaves"""
    support, brick_of, n = S.train_bricks(sigma, b, dilation)
    return support, brick_of, n, S.flags(support, brick_of, b), S.master_rows(sigma, coefficients, support, brick_of, b)


def finished(sigma, threshold):
    """sigma as finish(threshold) stores it"""
    s = np.asarray(sigma, dtype=np.float32)
    return np.where(s > np.float32(threshold), s, np.float32(0)).astype(np.float32)
