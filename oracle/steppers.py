"""CPU ORACLE (test infrastructure): numpy restatement of the reference's
integrator steppers and of one EPEC/PEC time step, operating in place on host
ParticleArrays (real particles only, integrator_cython.mako:103-104).

Pinned against the reference's own ``WCSPHStep`` / ``TransportVelocityStep``
Python methods by tests/golden/steppers.npz (tests/golden/make_golden.py).
"""


def wcsph_initialize(pa):
    """WCSPHStep.initialize  pysph/sph/integrator_step.py:51-61"""
    n = pa.get_number_of_particles(True)
    for a, b in (('x0', 'x'), ('y0', 'y'), ('z0', 'z'), ('u0', 'u'),
                 ('v0', 'v'), ('w0', 'w'), ('rho0', 'rho')):
        pa.properties[a][:n] = pa.properties[b][:n]


def wcsph_stage(pa, dt, stage):
    """WCSPHStep.stage1 (:63-76) / stage2 (:78-92)"""
    n = pa.get_number_of_particles(True)
    p = pa.properties
    f = 0.5 * dt if stage == 1 else dt
    for q, q0, aq in (('u', 'u0', 'au'), ('v', 'v0', 'av'), ('w', 'w0', 'aw'),
                      ('x', 'x0', 'ax'), ('y', 'y0', 'ay'), ('z', 'z0', 'az'),
                      ('rho', 'rho0', 'arho')):
        p[q][:n] = p[q0][:n] + f * p[aq][:n]


def tvf_stage1(pa, dt):
    """TransportVelocityStep.stage1  integrator_step.py:268-285"""
    n = pa.get_number_of_particles(True)
    p = pa.properties
    dtb2 = 0.5 * dt
    for q, aq in (('u', 'au'), ('v', 'av'), ('w', 'aw')):
        p[q][:n] += dtb2 * p[aq][:n]
    for qh, q, aq in (('uhat', 'u', 'auhat'), ('vhat', 'v', 'avhat'),
                      ('what', 'w', 'awhat')):
        p[qh][:n] = p[q][:n] + dtb2 * p[aq][:n]
    for x, qh in (('x', 'uhat'), ('y', 'vhat'), ('z', 'what')):
        p[x][:n] += dt * p[qh][:n]


def tvf_stage2(pa, dt):
    """TransportVelocityStep.stage2  integrator_step.py:287-299"""
    n = pa.get_number_of_particles(True)
    p = pa.properties
    dtb2 = 0.5 * dt
    for q, aq in (('u', 'au'), ('v', 'av'), ('w', 'aw')):
        p[q][:n] += dtb2 * p[aq][:n]
    p['vmag2'][:n] = p['u'][:n] * p['u'][:n] + p['v'][:n] * p['v'][:n] + \
        p['w'][:n] * p['w'][:n]


def epec_step(arrays, nnps, ev, t, dt, domain=None):
    """EPECIntegrator.one_timestep with WCSPHStep  (integrator.py:401-420)."""
    def accel():
        nnps.update()
        ev.compute(t, dt)

    def upd():
        if domain is not None:
            domain.update()
    for pa in arrays:
        wcsph_initialize(pa)
    accel()
    for pa in arrays:
        wcsph_stage(pa, dt, 1)
    upd()
    accel()
    for pa in arrays:
        wcsph_stage(pa, dt, 2)
    upd()


def pec_step_tvf(arrays, nnps, ev, t, dt, domain=None):
    """Integrator.one_timestep (PEC) with TransportVelocityStep
    (integrator.py:227-246)."""
    for pa in arrays:
        tvf_stage1(pa, dt)
    if domain is not None:
        domain.update()
    nnps.update()
    ev.compute(t, dt)
    for pa in arrays:
        tvf_stage2(pa, dt)
    if domain is not None:
        domain.update()


_SM = [('x', 'x0', 'ax'), ('y', 'y0', 'ay'), ('z', 'z0', 'az'), ('u', 'u0', 'au'),
       ('v', 'v0', 'av'), ('w', 'w0', 'aw'), ('rho', 'rho0', 'arho'),
       ('e', 'e0', 'ae'), ('s00', 's000', 'as00'), ('s01', 's010', 'as01'),
       ('s02', 's020', 'as02'), ('s11', 's110', 'as11'), ('s12', 's120', 'as12'),
       ('s22', 's220', 'as22')]


def solid_initialize(pa):
    """SolidMechStep.initialize  pysph/sph/integrator_step.py:175-197"""
    n = pa.get_number_of_particles(True)
    for q, q0, _ in _SM:
        pa.properties[q0][:n] = pa.properties[q][:n]


def solid_stage(pa, dt, stage):
    """SolidMechStep.stage1 (:199-226) / stage2 (:228-255)"""
    n = pa.get_number_of_particles(True)
    p = pa.properties
    f = 0.5 * dt if stage == 1 else dt
    for q, q0, aq in _SM:
        p[q][:n] = p[q0][:n] + f * p[aq][:n]


# ---------------------------------------------------------------------------
# EDACStep / EDACTVFStep (pysph/sph/wc/edac.py), GasDFluidStep and GSPHStep
# (pysph/sph/integrator_step.py), restated from the semantics cited in
# pysph_amd/csrc/sph_integrate.hip and include/sphhip.h.  Every product and every
# sum is rounded on its own (numpy has no fma).  Pinned bit-exactly to
# tests/golden/edac_steppers.npz, gasd_steppers.npz and gsph_steppers.npz.
# ---------------------------------------------------------------------------
_XU0 = [('x0', 'x'), ('y0', 'y'), ('z0', 'z'), ('u0', 'u'), ('v0', 'v'), ('w0', 'w')]


def edac_initialize(pa):
    """EDACStep.initialize (edac.py:95-105) == EDACTVFStep.initialize (:493-503)"""
    n = pa.get_number_of_particles(True)
    p = pa.properties
    for a, b in _XU0 + [('p0', 'p')]:
        p[a][:n] = p[b][:n]


def edac_stage(pa, dt, stage, tvf=False):
    """EDACStep.stage1 / stage2 (edac.py:107-133): velocities from au, positions from ax (u + the XSPH correction),
    the pressure from ap.  tvf=True: EDACTVFStep (:505-540), the positions move with uhat = u + f auhat instead."""
    n = pa.get_number_of_particles(True)
    p = pa.properties
    f = 0.5 * dt if stage == 1 else dt
    for q, q0, aq in (('u', 'u0', 'au'), ('v', 'v0', 'av'), ('w', 'w0', 'aw')):
        p[q][:n] = p[q0][:n] + f * p[aq][:n]
    if not tvf:
        for q, q0, aq in (('x', 'x0', 'ax'), ('y', 'y0', 'ay'), ('z', 'z0', 'az')):
            p[q][:n] = p[q0][:n] + f * p[aq][:n]
    else:
        for qh, q, aq in (('uhat', 'u', 'auhat'), ('vhat', 'v', 'avhat'), ('what', 'w', 'awhat')):
            p[qh][:n] = p[q][:n] + f * p[aq][:n]
        for q, q0, qh in (('x', 'x0', 'uhat'), ('y', 'y0', 'vhat'), ('z', 'z0', 'what')):
            p[q][:n] = p[q0][:n] + f * p[qh][:n]
    p['p'][:n] = p['p0'][:n] + f * p['ap'][:n]


def gasd_initialize(pa):
    """GasDFluidStep.initialize (integrator_step.py:353-378): the copies, ``converged`` cleared and ``omega`` set
    to 1 for the density iteration"""
    n = pa.get_number_of_particles(True)
    p = pa.properties
    for a, b in _XU0 + [('e0', 'e'), ('h0', 'h'), ('rho0', 'rho'), ('alpha10', 'alpha1'), ('alpha20', 'alpha2')]:
        p[a][:n] = p[b][:n]
    p['converged'][:n] = 0.0
    p['omega'][:n] = 1.0


def gasd_stage(pa, dt, stage):
    """GasDFluidStep.stage1 (:380-407, dt/2; h and rho predicted) / stage2 (:409-428, dt)"""
    n = pa.get_number_of_particles(True)
    p = pa.properties
    f = 0.5 * dt if stage == 1 else dt
    for q, q0, aq in (('u', 'u0', 'au'), ('v', 'v0', 'av'), ('w', 'w0', 'aw')):
        p[q][:n] = p[q0][:n] + f * p[aq][:n]
    for q, q0, vq in (('x', 'x0', 'u'), ('y', 'y0', 'v'), ('z', 'z0', 'w')):
        p[q][:n] = p[q0][:n] + f * p[vq][:n]
    p['e'][:n] = p['e0'][:n] + f * p['ae'][:n]
    if stage == 1:
        p['h'][:n] = p['h0'][:n] + f * p['ah'][:n]
        p['rho'][:n] = p['rho0'][:n] + f * p['arho'][:n]
    p['alpha1'][:n] = p['alpha10'][:n] + f * p['aalpha1'][:n]
    p['alpha2'][:n] = p['alpha20'][:n] + f * p['aalpha2'][:n]


def gsph_stage1(pa, dt):
    """GSPHStep.stage1 (integrator_step.py:433-449), the only stage: the energy and the positions move with the
    half-step velocities u* = u + dt/2 au"""
    n = pa.get_number_of_particles(True)
    p = pa.properties
    dtb2 = 0.5 * dt
    au, av, aw = p['au'][:n], p['av'][:n], p['aw'][:n]
    ustar = p['u'][:n] + dtb2 * au
    vstar = p['v'][:n] + dtb2 * av
    wstar = p['w'][:n] + dtb2 * aw
    p['u'][:n] = p['u'][:n] + dt * au
    p['v'][:n] = p['v'][:n] + dt * av
    p['w'][:n] = p['w'][:n] + dt * aw
    p['e'][:n] = p['e'][:n] + dt * (p['ae'][:n] - ustar * au - vstar * av - wstar * aw)
    p['x'][:n] = p['x'][:n] + dt * ustar
    p['y'][:n] = p['y'][:n] + dt * vstar
    p['z'][:n] = p['z'][:n] + dt * wstar
