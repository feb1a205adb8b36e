"""What the rigid-body moments and motion cost on the device, and what the host path costs.

Two shapes: ONE body of 52 020 particles (the body of profiles/scatter_time.json: 102 x 102 x 5 lattice points) and
10 000 bodies of 27 particles (3^3 lattice points each).  Per shape:

  moments   `sph_rigid_moments`: the chunk sums and the per-body algebra (two launches);
  motion    `sph_rigid_motion` over every row (one launch);
  host      the path a user had before: a user-defined equation whose ``reduce`` does the reference's numpy sums
            (one mask and 16 sums per body, then the per-body algebra) in an AccelerationEval with sync='auto' --
            wall-clock time of `compute`, which holds the push of the equation's inputs, the (trivial) launch, the
            pull of its outputs around the hook, the numpy pass and the push behind it.

Device numbers are PER-CALL TIMES IN A BACK-TO-BACK STREAM, not kernel times: one pair of events around a batch of
`--batch` calls issued from Python through the C-ABI (default 2000: a window of 15-70 ms, about 0.1 s of warm-up and
0.5-1 s of timed work per part), per-call time = interval / batch, medians over `--reps` windows.  At these sizes
the calls are launch-bound: `motion` costs the same at 52 020 and at 270 000 rows -- what is measured is the rate
at which launches can be enqueued and retired, which is also what a time step pays.  Host times: medians of
`--host-reps` calls (wall clock around `compute` and a synchronise).

    python tools/rigid_time.py [--reps 15 --batch 2000 --host-reps 3] [--out profiles/rigid_time.json] [--build-only]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def one_body():
    dx = 1.0 / 102
    g = (np.arange(102) + 0.5) * dx
    x, y, z = [a.ravel() for a in np.meshgrid(g, g[:5], g, indexing='ij')]
    return x, y, z, np.zeros(x.size, dtype=np.int32)


def many_bodies(nb=10000):
    c = np.arange(3) * 0.01
    lx, ly, lz = [a.ravel() for a in np.meshgrid(c, c, c, indexing='ij')]
    side = int(round(nb ** (1.0 / 3.0) + 0.5))
    b = np.arange(nb)
    ox, oy, oz = (b % side) * 0.05, ((b // side) % side) * 0.05, (b // (side * side)) * 0.05
    x = (ox[:, None] + lx[None, :]).ravel()
    y = (oy[:, None] + ly[None, :]).ravel()
    z = (oz[:, None] + lz[None, :]).ravel()
    return x, y, z, np.repeat(b, 27).astype(np.int32)


def make_array(shape, seed=1):
    from pysph_amd.particle_array import get_particle_array_rigid_body
    x, y, z, ids = one_body() if shape == 'one_body' else many_bodies()
    rng = np.random.default_rng(seed)
    n = x.size
    pa = get_particle_array_rigid_body(name='body', x=x, y=y, z=z, m=rng.uniform(0.5, 2.0, n), h=0.013 * np.ones(n),
                                       body_id=ids, fx=rng.normal(0, 1, n), fy=rng.normal(0, 1, n), fz=rng.normal(0, 1, n))
    pa.omega[:] = rng.normal(0, 1, pa.omega.size)
    return pa


def user_equation():
    """the reference's reduce pattern as a user would write it today: a mask and numpy sums per body on the host"""
    from pysph_amd.equations import Equation
    from pysph_amd.rigid_body import solve_symmetric3

    class HostMoments(Equation):
        def initialize(self, d_idx, d_au):
            d_au[d_idx] = 0.0

        def reduce(self, dst, t, dt):
            for b in range(int(dst.num_body[0])):
                cond = dst.body_id == b
                m, x, y, z = dst.m[cond], dst.x[cond], dst.y[cond], dst.z[cond]
                fx, fy, fz = dst.fx[cond], dst.fy[cond], dst.fz[cond]
                mass = np.sum(m)
                cx, cy, cz = np.sum(m * x) / mass, np.sum(m * y) / mass, np.sum(m * z) / mass
                ixx = np.sum(m * (y * y + z * z)) - (cy * cy + cz * cz) * mass
                iyy = np.sum(m * (x * x + z * z)) - (cx * cx + cz * cz) * mass
                izz = np.sum(m * (x * x + y * y)) - (cx * cx + cy * cy) * mass
                ixy = cx * cy * mass - np.sum(m * x * y)
                ixz = cx * cz * mass - np.sum(m * x * z)
                iyz = cy * cz * mass - np.sum(m * y * z)
                f = (np.sum(fx), np.sum(fy), np.sum(fz))
                tq = (np.sum(y * fz - z * fy) - (cy * f[2] - cz * f[1]), np.sum(z * fx - x * fz) - (cz * f[0] - cx * f[2]),
                      np.sum(x * fy - y * fx) - (cx * f[1] - cy * f[0]))
                dst.total_mass[b] = mass
                dst.cm[3 * b:3 * b + 3] = (cx, cy, cz)
                dst.mi[16 * b:16 * b + 9] = (ixx, ixy, ixz, ixy, iyy, iyz, ixz, iyz, izz)
                dst.force[3 * b:3 * b + 3] = f
                dst.ac[3 * b:3 * b + 3] = (f[0] / mass, f[1] / mass, f[2] / mass)
                dst.torque[3 * b:3 * b + 3] = tq
                wx, wy, wz = dst.omega[3 * b:3 * b + 3]
                lx, ly, lz = ixx * wx + ixy * wy + ixz * wz, ixy * wx + iyy * wy + iyz * wz, ixz * wx + iyz * wy + izz * wz
                dst.omega_dot[3 * b:3 * b + 3] = solve_symmetric3(
                    ixx, iyy, izz, ixy, ixz, iyz, tq[0] - (wy * lz - wz * ly), tq[1] - (wz * lx - wx * lz),
                    tq[2] - (wx * ly - wy * lx))
    return HostMoments(dest='body', sources=None)


def build_only():
    """the user equation's (trivial) generated family, compiled without a GPU"""
    from pysph_amd import kernels as K
    from pysph_amd.acceleration_eval import AccelerationEval, _CGroup
    from pysph_amd.equations import Group
    pa = make_array('many_bodies')
    kernel = K.CubicSpline(dim=3)
    a = AccelerationEval([pa], [Group(equations=[user_equation()])], kernel)
    return [len(_CGroup(g, {'body': 0}, {'body': pa}, K.kernel_id(kernel)).units) for g in a.equation_groups]


def measure(shape, args, torch, stream):
    from pysph_amd import device as dev
    from pysph_amd import kernels as K
    from pysph_amd.acceleration_eval import AccelerationEval, SPHCompiler
    from pysph_amd.equations import Group
    from pysph_amd.nnps import HipNNPS
    pa = make_array(shape)
    ctx = dev.HipContext(0, stream.cuda_stream)
    h = dev.attach(pa, ctx)
    h.push()
    h.rigid_setup()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.batch):
            fn()
        e1.record(stream)
        ctx.synchronize()
        return e0.elapsed_time(e1) / args.batch
    parts = dict(moments=h.rigid_moments, motion=h.rigid_motion)
    for _ in range(2 * args.batch):      # warm-up: code objects and the clock
        for fn in parts.values():
            fn()
    ctx.synchronize()
    runs = dict((k, []) for k in parts)
    for _ in range(args.reps):
        for k, fn in parts.items():
            runs[k].append(timed(fn))
    h.pull('cm')
    device_cm = pa.cm.copy()
    # the host path, in a context of its own
    pb = make_array(shape)
    ctx2 = dev.HipContext(0, stream.cuda_stream)
    kernel = K.CubicSpline(dim=3)
    a_eval = AccelerationEval([pb], [Group(equations=[user_equation()])], kernel)
    SPHCompiler(a_eval, ctx=ctx2, sync='auto').compile()
    a_eval.set_nnps(HipNNPS(3, [pb], radius_scale=kernel.radius_scale, ctx=ctx2))
    a_eval.compute(0.0, 1e-4)
    host = []
    for _ in range(args.host_reps):
        t0 = time.perf_counter()
        a_eval.compute(0.0, 1e-4)
        ctx2.synchronize()
        host.append(1e3 * (time.perf_counter() - t0))
    assert np.allclose(pb.cm, device_cm, rtol=1e-9, atol=1e-12)     # both paths computed the same thing
    med = dict((k, float(np.median(v))) for k, v in runs.items())
    med['host'] = float(np.median(host))
    out = dict(particles=pa.get_number_of_particles(), bodies=int(pa.num_body[0]),
               what='per-call ms in a back-to-back stream (launch-bound); host: wall clock of compute', median_ms=med,
               all_ms=dict([(k, [round(x, 5) for x in v]) for k, v in runs.items()] + [('host', [round(x, 3) for x in host])]),
               host_over_device_moments=med['host'] / med['moments'])
    ctx.close()
    ctx2.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--batch', type=int, default=2000, help='calls between one pair of events')
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--build-only', action='store_true', help='compile the generated family of the host path and exit')
    args = ap.parse_args()
    if args.build_only:
        print('units:', build_only())
        return
    import torch
    from pysph_amd import device as dev
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    result = dict(chunk=int(dev.load_library().sph_rigid_chunk()), reps=args.reps, batch=args.batch,
                  host_reps=args.host_reps)
    for shape in ('one_body', 'many_bodies'):
        result[shape] = measure(shape, args, torch, stream)
    print(json.dumps(result))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
