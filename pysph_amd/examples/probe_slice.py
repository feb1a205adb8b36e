"""Look at a running, device-resident dam break: every N steps interpolate
p, u, v, w onto the x-z mid-plane (y = 0) through ONE ``Interpolator`` that
shares the simulation's context (``sync=False``: the particle data never
leaves the GPU; one neighbour sweep carries all four fields) and save the
slices as ``slice_<step>.npz``.

    python -m pysph_amd.examples.probe_slice --dx 0.04 --steps 100 --every 20 --out slices
"""
import argparse
import os

import numpy as np

from . import dam_break_3d as db
from ..tools import Interpolator


def main():
    ap = argparse.ArgumentParser(description='x-z mid-plane slices of the 3-D dam break')
    ap.add_argument('--dx', type=float, default=0.04)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--every', type=int, default=20)
    ap.add_argument('--nx', type=int, default=161)
    ap.add_argument('--nz', type=int, default=51)
    ap.add_argument('--out', default='slices')
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    x, z = np.meshgrid(np.linspace(0.0, 3.22, args.nx), np.linspace(0.0, 1.0, args.nz), indexing='ij')
    state = {}

    def probe(step, t, arrays, ctx):
        if step % args.every:
            return
        if 'interp' not in state:
            state['interp'] = Interpolator(arrays, kernel=db.create_kernel(), x=x, y=np.zeros_like(x), z=z,
                                           method='shepard', ctx=ctx, sync=False)
        p, u, v, w = state['interp'].interpolate_many(['p', 'u', 'v', 'w'])
        path = os.path.join(args.out, 'slice_%05d.npz' % step)
        np.savez_compressed(path, t=t, x=x, z=z, p=p, u=u, v=v, w=w)
        print('step %d  t = %.5f  %s  max p = %.4g' % (step, t, path, p.max()))

    db.run(dx=args.dx, n_steps=args.steps, probe=probe)


if __name__ == '__main__':
    main()
