"""What the per-instance GPU tests share (tests/test_gpu_instance_*.py: cost parameters, subsystem parameters, routes, time
nominals): the output arrays a solve is compared on, the exact comparison, the headline scene, and the one check all four
make — an instance of a heterogeneous batch returns the bits of the same instance solved in a problem created with its
vector written into the descriptor.  Imported as `helpers` is; the files keep what differs between them: their scenes,
how they draw vectors, how a table is bound and how a vector is baked."""
import numpy as np

from ilqgames_amd import examples

KEYS = ("xs", "us", "P", "alpha", "costs", "iters", "status", "converged")


def to_numpy(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def headline():
    s = examples.modified_three_player_intersection()
    s.params.initial_alpha_scaling = 0.1          # the bench's line-search parameters
    s.params.expected_decrease_fraction = 0.001
    s.params.max_solver_iters = 25
    return s


def check_baked_equals_bound(hip, spec, dtype, make_bound, make_baked, vectors, B=12, seed=5, whole_batch_partner=False,
                             **solve_kw):
    """Instance b of a batch of B takes vectors[b % len(vectors)].  make_bound(table_rows) -> the problem with the table
    of those B rows bound; make_baked(vector) -> the spec with one vector written in.  Over every instance and every array
    of KEYS the bound solve equals the baked one bit for bit.  -> (the bound problem, its outputs, x0, b -> its vector)."""
    BV = len(vectors)
    x0 = examples.jittered_x0(spec, B, seed=seed + 1)
    which = np.arange(B) % BV
    prob = make_bound(vectors[which])
    out = {k: to_numpy(v) for k, v in prob.solve(x0, **solve_kw).items() if k in KEYS}
    row_program = prob.row_program()
    differ = False
    for v in range(BV):
        sel = np.nonzero(which == v)[0]
        ref_prob = hip.Problem(make_baked(vectors[v]), dtype)
        # deterministic solves: an instance's bits do not depend on its batch, the partner solves its instances alone;
        # otherwise the partner is a homogeneous batch of the same size (the same schedule)
        ref = ref_prob.solve(x0 if whole_batch_partner else x0[sel], **solve_kw)
        for k in KEYS:
            r = to_numpy(ref[k])
            r = r[sel] if whole_batch_partner else r
            assert same_bits(out[k][sel], r), (k, v, np.nonzero(np.any((out[k][sel] != r).reshape(len(sel), -1), axis=1))[0])
        if v == 0:
            ref0_prob, ref0_xs = ref_prob, to_numpy(ref["xs"])
        else:  # the same instance, from the same x0, under vector 0 and under vector v
            b = sel[0]
            under0 = ref0_xs[b] if whole_batch_partner else to_numpy(ref0_prob.solve(x0[b:b + 1], **solve_kw)["xs"])[0]
            differ = differ or not same_bits(out["xs"][b], under0)
    assert differ, "the vectors should lead to different trajectories"
    assert int(out["iters"].min()) > 0
    # declaring and binding touch neither the row program nor the static structure it matched: both are the descriptor's
    plain = hip.Problem(spec, dtype).row_program()
    assert np.array_equal(row_program[0], plain[0]) and row_program[1] == plain[1]
    return prob, out, x0, which
