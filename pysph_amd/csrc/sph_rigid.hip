// sph_rigid.hip -- rigid bodies on the device: moments, motion, steppers.
//
// Replaces the host reduction of RigidBodyMoments.reduce and the run-time indexed array constants of RigidBodyMotion /
// RK2StepRigidBody / EulerStepRigidBody (pysph/sph/rigid_body.py:69-230, 695-771).  The state of the bodies is a block of
// doubles in the layout of the reference's constants (pysph/base/utils.py:268-286); which body a row belongs to is the
// property body_id.  DESIGN.md section 7d.
//
// The sums of a body are taken over a BODY INDEX: the rows sorted by body id (stable), cut into chunks of at most
// SPH_RIGID_CHUNK entries that never span two bodies.  One wavefront sums one chunk (k_rigid_partials), one wavefront adds
// the chunk rows of one body and does the body's algebra (k_rigid_finish).  Nothing is added atomically: the order of
// every sum is fixed by the order of the body's own rows, so results repeat bit for bit from call to call and do not
// depend on which other bodies share the array.  Everything is fp64 whatever arith_f32 / record_f32 say: body state is
// storage precision.
#include <algorithm>
#include "sph_internal.h"

#define SPH_RIGID_CHUNK 256
static_assert(SPH_RIGID_CHUNK % 64 == 0, "a chunk is a whole number of wavefront strides");

// doubles per body of every field, and where a field starts in the state block (in units of nb)
static const int RIGID_WIDTH[SPH_RIGID_FIELD_COUNT] = {1, 3, 16, 3, 3, 3, 3, 3, 3, 3, 3};
static const int RIGID_OFFSET[SPH_RIGID_FIELD_COUNT + 1] = {0, 1, 4, 20, 23, 26, 29, 32, 35, 38, 41, 44};

struct RigidPtrs { // the fields of one state block
    double *total_mass, *cm, *mi, *force, *torque, *vc, *ac, *vc0, *omega, *omega0, *omega_dot;
};

static RigidPtrs rigid_ptrs(const RigidState &R)
{
    double *s = R.state.as<double>();
    const size_t nb = (size_t)R.nb;
    RigidPtrs p;
    p.total_mass = s + RIGID_OFFSET[SPH_RIGID_TOTAL_MASS] * nb;
    p.cm = s + RIGID_OFFSET[SPH_RIGID_CM] * nb;
    p.mi = s + RIGID_OFFSET[SPH_RIGID_MI] * nb;
    p.force = s + RIGID_OFFSET[SPH_RIGID_FORCE] * nb;
    p.torque = s + RIGID_OFFSET[SPH_RIGID_TORQUE] * nb;
    p.vc = s + RIGID_OFFSET[SPH_RIGID_VC] * nb;
    p.ac = s + RIGID_OFFSET[SPH_RIGID_AC] * nb;
    p.vc0 = s + RIGID_OFFSET[SPH_RIGID_VC0] * nb;
    p.omega = s + RIGID_OFFSET[SPH_RIGID_OMEGA] * nb;
    p.omega0 = s + RIGID_OFFSET[SPH_RIGID_OMEGA0] * nb;
    p.omega_dot = s + RIGID_OFFSET[SPH_RIGID_OMEGA_DOT] * nb;
    return p;
}

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
// One wavefront per chunk.  partial[chunk][16]: sum of m, m x, m y, m z, m (y^2 + z^2), m (x^2 + z^2), m (x^2 + y^2),
// m x y, m x z, m y z, fx, fy, fz, (r x f)_x, (r x f)_y, (r x f)_z over the chunk's rows, all about the origin
// (rigid_body.py:98-122).  A lane takes entries lane, lane + 64, ... of its chunk in that order; the lanes are added by the
// fixed xor tree.
__global__ __launch_bounds__(256) void k_rigid_partials(const uint32_t *__restrict__ order, const uint32_t *__restrict__ chunk,
                                                        size_t nchunks, size_t n, const double *__restrict__ x,
                                                        const double *__restrict__ y, const double *__restrict__ z,
                                                        const double *__restrict__ m, const double *__restrict__ fx,
                                                        const double *__restrict__ fy, const double *__restrict__ fz,
                                                        double *__restrict__ partial)
{
    const size_t k = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); // wave-uniform
    const uint32_t lane = threadIdx.x & 63;
    if (k >= nchunks) return;
    const uint32_t beg = chunk[2 * k], cnt = chunk[2 * k + 1];
    double s[16];
#pragma unroll
    for (int q = 0; q < 16; q++) s[q] = 0.0;
    for (uint32_t j = lane; j < cnt; j += 64) {
        const size_t i = order[beg + j];
        if (i >= n) continue; // (an index is checked when it is built; never read outside the array)
        const double px = x[i], py = y[i], pz = z[i], pm = m[i], gx = fx[i], gy = fy[i], gz = fz[i];
        s[0] += pm;
        s[1] += pm * px;
        s[2] += pm * py;
        s[3] += pm * pz;
        s[4] += pm * (py * py + pz * pz);
        s[5] += pm * (px * px + pz * pz);
        s[6] += pm * (px * px + py * py);
        s[7] += pm * px * py;
        s[8] += pm * px * pz;
        s[9] += pm * py * pz;
        s[10] += gx;
        s[11] += gy;
        s[12] += gz;
        s[13] += py * gz - pz * gy;
        s[14] += pz * gx - px * gz;
        s[15] += px * gy - py * gx;
    }
#pragma unroll
    for (int q = 0; q < 16; q++)
        for (int o = 32; o > 0; o >>= 1) s[q] += __shfl_xor(s[q], o, 64);
    if (lane == 0) {
        double *out = partial + k * 16;
#pragma unroll
        for (int q = 0; q < 16; q++) out[q] = s[q];
    }
}

// One wavefront per body.  Lane (sub, q) = (lane / 16, lane % 16) adds quantity q of the body's chunk rows sub, sub + 4, ...
// in chunk order; the four sub-sums are added by the xor tree.  Lane 0 then does the algebra of rigid_body.py:128-207.
__global__ __launch_bounds__(256) void k_rigid_finish(const uint32_t *__restrict__ chunk_start, const double *__restrict__ partial,
                                                      int nb, RigidPtrs S)
{
    const int b = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)); // wave-uniform
    const uint32_t lane = threadIdx.x & 63;
    if (b >= nb) return;
    const uint32_t c0 = chunk_start[b], c1 = chunk_start[b + 1];
    const uint32_t q = lane & 15, sub = lane >> 4;
    double s = 0.0;
    for (uint32_t r = c0 + sub; r < c1; r += 4) s += partial[(size_t)r * 16 + q];
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    double a[16];
#pragma unroll
    for (int k = 0; k < 16; k++) a[k] = __shfl(s, k, 64);
    if (lane != 0) return;
    const double mass = a[0];
    const double cx = a[1] / mass, cy = a[2] / mass, cz = a[3] / mass;
    // inertia about the centre of mass: parallel-axis theorem on the moments about the origin
    const double ixx = a[4] - (cy * cy + cz * cz) * mass;
    const double iyy = a[5] - (cx * cx + cz * cz) * mass;
    const double izz = a[6] - (cx * cx + cy * cy) * mass;
    const double ixy = cx * cy * mass - a[7];
    const double ixz = cx * cz * mass - a[8];
    const double iyz = cy * cz * mass - a[9];
    const double fx = a[10], fy = a[11], fz = a[12];
    // torque about the centre of mass: sum (r x f) - cm x F
    const double tx = a[13] - (cy * fz - cz * fy);
    const double ty = a[14] - (cz * fx - cx * fz);
    const double tz = a[15] - (cx * fy - cy * fx);
    S.total_mass[b] = mass;
    double *cm = S.cm + 3 * (size_t)b, *mi = S.mi + 16 * (size_t)b;
    cm[0] = cx; cm[1] = cy; cm[2] = cz;
    mi[0] = ixx; mi[1] = ixy; mi[2] = ixz;
    mi[3] = ixy; mi[4] = iyy; mi[5] = iyz;
    mi[6] = ixz; mi[7] = iyz; mi[8] = izz;
    // (slots 9..15 keep the sums the reference leaves there: -sum m y z, the force, the torque about the origin)
    mi[9] = -a[9]; mi[10] = fx; mi[11] = fy; mi[12] = fz; mi[13] = a[13]; mi[14] = a[14]; mi[15] = a[15];
    double *force = S.force + 3 * (size_t)b, *ac = S.ac + 3 * (size_t)b, *torque = S.torque + 3 * (size_t)b;
    force[0] = fx; force[1] = fy; force[2] = fz;
    ac[0] = fx / mass; ac[1] = fy / mass; ac[2] = fz / mass;
    torque[0] = tx; torque[1] = ty; torque[2] = tz;
    // Euler's equation: omega_dot = I^-1 (tau - omega x (I omega)), I symmetric: adjugate over determinant
    const double *om = S.omega + 3 * (size_t)b;
    const double wx = om[0], wy = om[1], wz = om[2];
    const double lx = ixx * wx + ixy * wy + ixz * wz;
    const double ly = ixy * wx + iyy * wy + iyz * wz;
    const double lz = ixz * wx + iyz * wy + izz * wz;
    const double rx = tx - (wy * lz - wz * ly);
    const double ry = ty - (wz * lx - wx * lz);
    const double rz = tz - (wx * ly - wy * lx);
    const double a00 = iyy * izz - iyz * iyz, a01 = ixz * iyz - ixy * izz, a02 = ixy * iyz - ixz * iyy;
    const double a11 = ixx * izz - ixz * ixz, a12 = ixy * ixz - ixx * iyz, a22 = ixx * iyy - ixy * ixy;
    const double rdet = 1.0 / (ixx * a00 + ixy * a01 + ixz * a02);
    double *od = S.omega_dot + 3 * (size_t)b;
    od[0] = (a00 * rx + a01 * ry + a02 * rz) * rdet;
    od[1] = (a01 * rx + a11 * ry + a12 * rz) * rdet;
    od[2] = (a02 * rx + a12 * ry + a22 * rz) * rdet;
}

// (u, v, w) = vc + omega x (r - cm) of the row's body (rigid_body.py:215-229).  The motion needs no body index, so nothing
// has validated body_id for it: a row whose id is outside [0, nb) keeps its u, v, w (the state is never read out of
// bounds); sph_rigid_moments reports such a row the next time it builds the index.
__global__ __launch_bounds__(256) void k_rigid_motion(size_t start, size_t stop, int nb, const double *__restrict__ body_id,
                                                      const double *__restrict__ x, const double *__restrict__ y,
                                                      const double *__restrict__ z, double *__restrict__ u,
                                                      double *__restrict__ v, double *__restrict__ w,
                                                      const double *__restrict__ cm, const double *__restrict__ vc,
                                                      const double *__restrict__ omega)
{
    const size_t i = start + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= stop) return;
    const long b = (long)body_id[i];
    if (b < 0 || b >= nb) return; // (never read outside the state; the index build reports such an id)
    const size_t base = 3 * (size_t)b;
    const double wx = omega[base], wy = omega[base + 1], wz = omega[base + 2];
    const double rx = x[i] - cm[base], ry = y[i] - cm[base + 1], rz = z[i] - cm[base + 2];
    u[i] = vc[base] + wy * rz - wz * ry;
    v[i] = vc[base + 1] + wz * rx - wx * rz;
    w[i] = vc[base + 2] + wx * ry - wy * rx;
}

struct RigidStageArgs {
    int stepper, stage;
    double dt;
    size_t n;
    double *x, *y, *z, *x0, *y0, *z0;
    const double *u, *v, *w;
};

// the per-particle half of a stage (rigid_body.py:713-715, 731-733, 750-752, 768-770)
__global__ __launch_bounds__(256) void k_rigid_stage(RigidStageArgs a)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    if (a.stepper == SPH_STEP_RIGID_EULER) {
        a.x[i] += a.dt * a.u[i];
        a.y[i] += a.dt * a.v[i];
        a.z[i] += a.dt * a.w[i];
    } else if (a.stage == 0) {
        a.x0[i] = a.x[i]; a.y0[i] = a.y[i]; a.z0[i] = a.z[i];
    } else {
        const double f = a.stage == 1 ? 0.5 * a.dt : a.dt;
        a.x[i] = a.x0[i] + f * a.u[i];
        a.y[i] = a.y0[i] + f * a.v[i];
        a.z[i] = a.z0[i] + f * a.w[i];
    }
}

// ... and the per-body half, what the reference does inside `if d_idx == 0`: one thread per component of a body.  No
// particle thread of a stage reads vc or omega, so the two launches are independent.
__global__ __launch_bounds__(256) void k_rigid_stage_bodies(int stepper, int stage, double dt, size_t n3, RigidPtrs S)
{
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n3) return;
    if (stepper == SPH_STEP_RIGID_EULER) {
        S.vc[k] += S.ac[k] * dt;
        S.omega[k] += S.omega_dot[k] * dt;
    } else if (stage == 0) {
        S.vc0[k] = S.vc[k];
        S.omega0[k] = S.omega[k];
    } else {
        const double f = stage == 1 ? 0.5 * dt : dt;
        S.vc[k] = S.vc0[k] + S.ac[k] * f;
        S.omega[k] = S.omega0[k] + S.omega_dot[k] * f;
    }
}

// ---------------------------------------------------------------------------
// the body index
// ---------------------------------------------------------------------------
static int rigid_check(sph_ctx *c, int id, const char *who, bool need_state = true)
{
    if (!c) { sph_set_error("%s: ctx is NULL", who); return SPH_ERR_ARG; }
    if (id < 0 || id >= SPH_MAX_ARRAYS) { sph_set_error("%s: bad array id %d", who, id); return SPH_ERR_ARG; }
    if (!c->arr[id].used) { sph_set_error("%s: array %d was never sized (sph_array_resize)", who, id); return SPH_ERR_STATE; }
    if (need_state && c->rigid[id].nb <= 0) { sph_set_error("%s: array %d has no bodies (call sph_rigid_setup first)", who, id); return SPH_ERR_STATE; }
    return SPH_OK;
}

// order / start (host) -> device, with the chunk tables.  start is checked here: every body has rows, the segments tile
// [0, n); order: every entry is a row of the array.
static int rigid_take_index(sph_ctx *c, int id, const uint32_t *order, const uint32_t *start)
{
    DevArray &A = c->arr[id];
    RigidState &R = c->rigid[id];
    const size_t n = A.n;
    const int nb = R.nb;
    if (start[0] != 0 || start[nb] != n) { sph_set_error("body index of array %d: the segments cover %u..%u of %zu rows", id, start[0], start[nb], n); return SPH_ERR_ARG; }
    for (int b = 0; b < nb; b++)
        if (start[b + 1] <= start[b]) { sph_set_error("body index of array %d: body %d has no particles", id, b); return SPH_ERR_ARG; }
    for (size_t i = 0; i < n; i++)
        if (order[i] >= n) { sph_set_error("body index of array %d: row %u out of range (n=%zu)", id, order[i], n); return SPH_ERR_ARG; }
    std::vector<uint32_t> chunk, chunk_start((size_t)nb + 1);
    for (int b = 0; b < nb; b++) {
        chunk_start[b] = (uint32_t)(chunk.size() / 2);
        for (uint32_t p = start[b]; p < start[b + 1]; p += SPH_RIGID_CHUNK) {
            chunk.push_back(p);
            chunk.push_back(std::min<uint32_t>(SPH_RIGID_CHUNK, start[b + 1] - p));
        }
    }
    chunk_start[nb] = (uint32_t)(chunk.size() / 2);
    R.nchunks = chunk.size() / 2;
    SPH_TRY(R.order.reserve(n * sizeof(uint32_t)));
    SPH_TRY(R.chunk.reserve(chunk.size() * sizeof(uint32_t)));
    SPH_TRY(R.chunk_start.reserve(chunk_start.size() * sizeof(uint32_t)));
    SPH_TRY(R.partial.reserve(R.nchunks * 16 * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(R.order.ptr, order, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(R.chunk.ptr, chunk.data(), chunk.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(R.chunk_start.ptr, chunk_start.data(), chunk_start.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream)); // the host vectors go out of scope
    R.index_epoch = A.rows_epoch;
    R.index_built = true;
    return SPH_OK;
}

// the index from the body_id column as it lies on the device: one pull, a counting sort on the host (stable in row order)
static int rigid_build_index(sph_ctx *c, int id)
{
    DevArray &A = c->arr[id];
    RigidState &R = c->rigid[id];
    const size_t n = A.n;
    const int nb = R.nb;
    if (R.body_prop < 0 || !A.prop[R.body_prop]) { sph_set_error("body index of array %d: the array has no body_id column on the device", id); return SPH_ERR_MISSING_PROP; }
    std::vector<double> col(n);
    if (n) {
        HIP_TRY(hipMemcpyAsync(col.data(), A.prop[R.body_prop], n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    std::vector<uint32_t> start((size_t)nb + 1, 0), order(n);
    for (size_t i = 0; i < n; i++) {
        const double v = col[i];
        if (!(v >= 0.0 && v < (double)nb) || v != (double)(long)v) {
            sph_set_error("body index of array %d: row %zu has body id %g, outside [0, %d)", id, i, v, nb);
            return SPH_ERR_ARG;
        }
        start[(size_t)v + 1]++;
    }
    for (int b = 0; b < nb; b++) start[b + 1] += start[b];
    std::vector<uint32_t> cur(start.begin(), start.end() - 1);
    for (size_t i = 0; i < n; i++) order[cur[(size_t)col[i]]++] = (uint32_t)i;
    return rigid_take_index(c, id, order.data(), start.data());
}

static int rigid_need_index(sph_ctx *c, int id)
{
    const DevArray &A = c->arr[id];
    const RigidState &R = c->rigid[id];
    if (R.index_built && R.index_epoch == A.rows_epoch) return SPH_OK; // (every change of n bumps rows_epoch, too)
    return rigid_build_index(c, id);
}

// ---------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------
extern "C" int sph_rigid_chunk(void) { return SPH_RIGID_CHUNK; }

extern "C" int sph_rigid_setup(sph_ctx *c, int id, int nbody, const uint32_t *order, const uint32_t *start)
{
    SPH_TRY(rigid_check(c, id, "sph_rigid_setup", false));
    if (nbody <= 0) { sph_set_error("sph_rigid_setup: %d bodies", nbody); return SPH_ERR_ARG; }
    if ((order == nullptr) != (start == nullptr)) { sph_set_error("sph_rigid_setup: order and start come together"); return SPH_ERR_ARG; }
    HIP_TRY(hipSetDevice(c->device));
    RigidState &R = c->rigid[id];
    const int body_prop = sph_prop_register("body_id");
    if (body_prop < 0) return body_prop;
    SPH_TRY(sph_array_ensure_prop(c, id, body_prop));
    if (R.nb != nbody) {
        const size_t bytes = (size_t)RIGID_OFFSET[SPH_RIGID_FIELD_COUNT] * nbody * sizeof(double);
        SPH_TRY(R.state.reserve(bytes));
        HIP_TRY(hipMemsetAsync(R.state.ptr, 0, bytes, c->stream));
        R.nb = nbody;
        R.index_built = false;
    }
    R.body_prop = body_prop;
    if (order) return rigid_take_index(c, id, order, start);
    R.index_built = false;
    return SPH_OK;
}

static int rigid_field(sph_ctx *c, int id, int field, size_t n, const char *who, double **ptr)
{
    SPH_TRY(rigid_check(c, id, who));
    const RigidState &R = c->rigid[id];
    if (field < 0 || field >= SPH_RIGID_FIELD_COUNT) { sph_set_error("%s: unknown field %d", who, field); return SPH_ERR_ARG; }
    const size_t want = (size_t)RIGID_WIDTH[field] * R.nb;
    if (n != want) { sph_set_error("%s: field %d holds %zu values for %d bodies, not %zu", who, field, want, R.nb, n); return SPH_ERR_ARG; }
    *ptr = R.state.as<double>() + (size_t)RIGID_OFFSET[field] * R.nb;
    return SPH_OK;
}

extern "C" int sph_rigid_state_push(sph_ctx *c, int id, int field, const double *host, size_t n)
{
    double *p = nullptr;
    SPH_TRY(rigid_field(c, id, field, n, "sph_rigid_state_push", &p));
    if (!host) { sph_set_error("sph_rigid_state_push: host is NULL"); return SPH_ERR_ARG; }
    HIP_TRY(hipMemcpyAsync(p, host, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream)); // (pageable host memory: the caller may reuse `host`)
    return SPH_OK;
}

extern "C" int sph_rigid_state_pull(sph_ctx *c, int id, int field, double *host, size_t n)
{
    double *p = nullptr;
    SPH_TRY(rigid_field(c, id, field, n, "sph_rigid_state_pull", &p));
    if (!host) { sph_set_error("sph_rigid_state_pull: host is NULL"); return SPH_ERR_ARG; }
    HIP_TRY(hipMemcpyAsync(host, p, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SPH_OK;
}

extern "C" int sph_rigid_moments(sph_ctx *c, int id)
{
    SPH_TRY(rigid_check(c, id, "sph_rigid_moments"));
    HIP_TRY(hipSetDevice(c->device));
    DevArray &A = c->arr[id];
    RigidState &R = c->rigid[id];
    const char *names[] = {"fx", "fy", "fz"};
    int f[3];
    for (int k = 0; k < 3; k++) {
        f[k] = sph_prop_register(names[k]);
        if (f[k] < 0) return f[k];
        SPH_TRY(sph_array_ensure_prop(c, id, f[k]));
    }
    for (int p : {SPH_X, SPH_Y, SPH_Z, SPH_M}) SPH_TRY(sph_array_ensure_prop(c, id, p));
    SPH_TRY(rigid_need_index(c, id));
    hipLaunchKernelGGL(k_rigid_partials, dim3(div_up(R.nchunks, 4)), dim3(256), 0, c->stream, R.order.as<uint32_t>(),
                       R.chunk.as<uint32_t>(), R.nchunks, A.n, A.prop[SPH_X], A.prop[SPH_Y], A.prop[SPH_Z], A.prop[SPH_M],
                       A.prop[f[0]], A.prop[f[1]], A.prop[f[2]], R.partial.as<double>());
    hipLaunchKernelGGL(k_rigid_finish, dim3(div_up((size_t)R.nb, 4)), dim3(256), 0, c->stream, R.chunk_start.as<uint32_t>(),
                       R.partial.as<double>(), R.nb, rigid_ptrs(R));
    return SPH_OK;
}

extern "C" int sph_rigid_motion(sph_ctx *c, int id, int real_only, long start, long stop)
{
    SPH_TRY(rigid_check(c, id, "sph_rigid_motion"));
    HIP_TRY(hipSetDevice(c->device));
    DevArray &A = c->arr[id];
    RigidState &R = c->rigid[id];
    for (int p : {(int)SPH_X, (int)SPH_Y, (int)SPH_Z, (int)SPH_U, (int)SPH_V, (int)SPH_W, R.body_prop}) SPH_TRY(sph_array_ensure_prop(c, id, p));
    const size_t n = real_only ? A.n_real : A.n;
    if (start < 0) { sph_set_error("sph_rigid_motion: start %ld", start); return SPH_ERR_ARG; }
    const size_t lo = (size_t)start, hi = stop < 0 ? n : std::min(n, (size_t)stop);
    if (lo >= hi) return SPH_OK;
    const RigidPtrs S = rigid_ptrs(R);
    hipLaunchKernelGGL(k_rigid_motion, dim3(div_up(hi - lo, 256)), dim3(256), 0, c->stream, lo, hi, R.nb, A.prop[R.body_prop],
                       A.prop[SPH_X], A.prop[SPH_Y], A.prop[SPH_Z], A.prop[SPH_U], A.prop[SPH_V], A.prop[SPH_W], S.cm, S.vc, S.omega);
    return SPH_OK;
}

int sph_rigid_stage(sph_ctx *c, int id, int stepper, int stage, double dt)
{
    SPH_TRY(rigid_check(c, id, "sph_integrate_stage (rigid body stepper)"));
    if (stepper == SPH_STEP_RIGID_EULER && stage != 1) return SPH_OK; // EulerStepRigidBody has stage1 only
    DevArray &A = c->arr[id];
    RigidState &R = c->rigid[id];
    for (int p : {SPH_X, SPH_Y, SPH_Z, SPH_U, SPH_V, SPH_W, SPH_X0, SPH_Y0, SPH_Z0}) SPH_TRY(sph_array_ensure_prop(c, id, p));
    if (A.n_real == 0) return SPH_OK; // (the reference updates the bodies in the thread of particle 0)
    RigidStageArgs a;
    a.stepper = stepper; a.stage = stage; a.dt = dt; a.n = A.n_real;
    a.x = A.prop[SPH_X]; a.y = A.prop[SPH_Y]; a.z = A.prop[SPH_Z];
    a.x0 = A.prop[SPH_X0]; a.y0 = A.prop[SPH_Y0]; a.z0 = A.prop[SPH_Z0];
    a.u = A.prop[SPH_U]; a.v = A.prop[SPH_V]; a.w = A.prop[SPH_W];
    ScopedTimer tm(c, T_STAGE);
    hipLaunchKernelGGL(k_rigid_stage, dim3(div_up(A.n_real, 256)), dim3(256), 0, c->stream, a);
    const size_t n3 = 3 * (size_t)R.nb;
    hipLaunchKernelGGL(k_rigid_stage_bodies, dim3(div_up(n3, 256)), dim3(256), 0, c->stream, stepper, stage, dt, n3, rigid_ptrs(R));
    if (stage > 0) { c->nnps_valid = false; } // positions moved
    return SPH_OK;
}
