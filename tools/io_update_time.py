"""Time one InletBase.update + OutletBase.update pair on the channel example's
particles at about a million fluid particles with a few thousand rows crossing
each interface: the device path (pysph_amd/inlet_outlet.py) against the same
update made through the host-side structural helpers (extract_particles,
append_parray, remove_particles, DeviceProperty get / set: the `_HostInlet` /
`_HostOutlet` of tests/test_inlet_outlet.py), on the same state, alternating,
after a warm-up.  Device events around the pair and the host clock around the
same region (the region ends in a synchronise); the bytes that crossed PCIe as
property data are counted at the library boundary (sph_array_push / _pull).

    python tools/io_update_time.py [--nx 100 --ny 100 --nz 100 --reps 5] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]


class Traffic(object):
    """counts what sph_array_push / sph_array_pull move while installed"""

    def __init__(self, lib):
        self.lib, self.bytes, self.calls = lib, 0, 0

    def __enter__(self):
        self.saved = (self.lib.sph_array_push, self.lib.sph_array_pull)

        def wrap(fn):
            def counted(ctx, aid, prop, host, offset, n):
                self.bytes += 8 * int(n)
                self.calls += 1
                return fn(ctx, aid, prop, host, offset, n)
            return counted
        self.lib.sph_array_push, self.lib.sph_array_pull = wrap(self.saved[0]), wrap(self.saved[1])
        return self

    def __exit__(self, *exc):
        self.lib.sph_array_push, self.lib.sph_array_pull = self.saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=100)
    ap.add_argument('--ny', type=int, default=100)
    ap.add_argument('--nz', type=int, default=100)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--breakdown', action='store_true',
                    help='also run the device path once with a synchronise after every helper call and print where the time goes')
    args = ap.parse_args()
    import torch
    import test_inlet_outlet as T
    from pysph_amd import device as dev
    from pysph_amd.examples import channel_flow as cf
    dx, n_io = 0.01, 4
    arrays = cf.create_particles(dx, args.nx, args.ny, args.nz, n_io=n_io, phases=4, outlet_filled=True)
    by_name = dict((pa.name, pa) for pa in arrays)
    for pa in arrays[:3]:
        pa.x += 0.13 * dx           # the last staggered group of every block is now across its interface / far end
    saved = [dict((k, v.copy()) for k, v in pa.properties.items()) for pa in arrays]
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = dev.HipContext(0, stream.cuda_stream)
    for p in ('gid', 'ioid', 'disp'):
        dev.prop_register(p)
    for pa in arrays:
        dev.attach(pa, ctx).push()
    iom = cf.create_manager(dx, args.nx)
    iom.setup_iom(3, None)
    iom.active_stages = [1]
    device_ios = iom.get_inlet_outlet(by_name)
    for info in iom.inletinfo + iom.outletinfo:
        info.length = n_io * dx
    host_ios = [T._HostInlet(device_ios[0], []), T._HostOutlet(device_ios[1], [])]

    def restore():
        for pa, props in zip(arrays, saved):
            for k, v in props.items():
                # (into the buffer the property has, head-room included, when it fits: a run in its steady state
                # does not allocate host arrays, and the timed region should not either)
                # (the host-side helpers of the other path leave exact-size arrays behind: give them the head-room a
                # device-path run has after its first growth, or the timed region would free and map 280 MB of host memory)
                arr = pa.properties[k]
                base = arr.base if isinstance(arr.base, np.ndarray) and arr.base.dtype == v.dtype else arr
                room = v.size + v.size // 8 + 64 * (v.size // max(props['x'].size, 1) or 1)
                if base.size < room:
                    base = np.zeros(room, dtype=v.dtype)
                pa.properties[k] = base[:v.size]
                pa.properties[k][:] = v
            pa._n = props['x'].size
            pa.set_num_real_particles(pa._n)
            pa.gpu._sync_size()
            pa.gpu.push()
        ctx.synchronize()

    def one(ios):
        restore()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with Traffic(ctx.lib) as tr:
            e0.record(stream)
            t0 = time.perf_counter()
            for io in ios:
                io.update(0.0, 1e-4, 1)
            e1.record(stream)
            ctx.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
        sizes = dict((pa.name, pa.gpu.get_number_of_particles()) for pa in arrays)
        return dict(event_ms=e0.elapsed_time(e1), wall_ms=wall, pcie_property_bytes=tr.bytes, pcie_property_copies=tr.calls,
                    sizes=sizes)

    n0 = dict((pa.name, pa.get_number_of_particles()) for pa in arrays)
    # warm-up: both paths once (code objects, allocations), then a burst of device work for the clock
    one(device_ios)
    one(host_ios)
    for _ in range(300):
        arrays[0].gpu.classify_plane((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), read=False)
    ctx.synchronize()
    runs = {'device': [], 'host': []}
    for _ in range(args.reps):
        runs['device'].append(one(device_ios))
        runs['host'].append(one(host_ios))
    crossing = dict(inlet_to_fluid=device_ios[0].last_counts[0], fluid_to_outlet=device_ios[1].last_counts[1][1],
                    deleted_from_outlet=device_ios[1].last_counts[0][2])
    assert runs['device'][-1]['sizes'] == runs['host'][-1]['sizes']
    result = dict(particles=n0, crossing=crossing, reps=args.reps)
    for k, rs in runs.items():
        result[k] = dict(event_ms_median=float(np.median([r['event_ms'] for r in rs])),
                         event_ms_all=[round(r['event_ms'], 4) for r in rs],
                         wall_ms_median=float(np.median([r['wall_ms'] for r in rs])),
                         pcie_property_bytes=rs[-1]['pcie_property_bytes'],
                         pcie_property_copies=rs[-1]['pcie_property_copies'])
    result['sizes_after'] = runs['device'][-1]['sizes']
    if args.breakdown:
        spent = {}

        def timed(name, fn, sync):
            def wrapper(*a, **kw):
                t0 = time.perf_counter()
                out = fn(*a, **kw)
                if sync:
                    ctx.synchronize()
                spent[name] = spent.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
                return out
            return wrapper
        H = dev.HipDeviceHelper
        keep = {}
        for name, sync in (('classify_plane', True), ('transfer_selected', True), ('shift_selected', True),
                           ('remove_selected', True), ('_host_follow', False), ('_transfer_ids', False),
                           ('device_props', False)):
            keep[name] = getattr(H, name)
            setattr(H, name, timed(name, keep[name], sync))
        keep['read_io_counts'] = H.__dict__['read_io_counts']
        H.read_io_counts = staticmethod(timed('read_io_counts', H.read_io_counts, True))
        total = one(device_ios)['wall_ms']
        for name, fn in keep.items():
            setattr(H, name, fn)
        result['breakdown_ms'] = dict((k, round(v, 3)) for k, v in sorted(spent.items()))
        result['breakdown_ms']['pair_with_synchronises'] = round(total, 3)
    print(json.dumps(result))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
    ctx.close()


if __name__ == '__main__':
    main()
