// device_functions_more.hip -- TEST ONLY: the probes of device_functions.hip for the smoothing kernels 5..10
// (SphKernel<5..10>::w/dw/dwq with the dimension argument, pair_geom, pair_w, pair_gradfac, pair_gradh), one value per
// thread, for tests/test_more_kernels_gpu.py.  Built with the flags of pysph_amd/csrc/Makefile (tests/more_kernels.py)
// so that contraction behaves as in the product.
//
// Every entry point takes HOST arrays, does its own hipMalloc / copy / launch / copy back and returns the first
// HIP error (0: fine).  `f32` selects float arrays and float arithmetic.
#include "sph_pair.h"

#include <cstddef>
#include <vector>

namespace {

// what pair_geom reads of its argument struct
struct ProbeArgs {
    double hu, h1u, facu, epsu;
    KernelConst k;
};

constexpr int PAIR_OUT = 10; // rij rinv hij h1 q fac eps | pair_w pair_gradfac pair_gradh

template <int KK, bool INSUP, class T>
__global__ void k_kernel(int n, int dim, const T *q, T *w, T *dw, T *dwq)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const T qi = q[i];
    w[i] = SphKernel<KK>::template w<INSUP>(qi, dim);
    dw[i] = SphKernel<KK>::template dw<INSUP>(qi, dim);
    dwq[i] = SphKernel<KK>::template dwq<INSUP>(qi, dim);
}

template <int KK, bool UH, class T>
__global__ void k_pair(int n, const T *r2, const T *hi, const T *hj, ProbeArgs a, T *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    real4<T> pi, pj;
    pi.x = T(1); pi.y = T(2); pi.z = T(3); pi.w = hi[i];
    pj.x = T(0.5); pj.y = T(1); pj.z = T(1.5); pj.w = hj[i];
    PairGeomT<T> g;
    pair_geom<KK, UH, T>(g, pi, pj, r2[i], a);
    const size_t N = (size_t)n;
    out[0 * N + i] = g.rij;
    out[1 * N + i] = g.rinv;
    out[2 * N + i] = g.hij;
    out[3 * N + i] = g.h1;
    out[4 * N + i] = g.q;
    out[5 * N + i] = g.fac;
    out[6 * N + i] = g.eps;
    out[7 * N + i] = pair_w<KK, UH, T>(g);
    out[8 * N + i] = pair_gradfac<KK, UH, T>(g);
    out[9 * N + i] = pair_gradh<KK, UH, T>(g, a.k.dim);
}

// device copies of host arrays; outputs go back in the destructor's stead through pull()
struct Bufs {
    std::vector<void *> ptrs;
    hipError_t err = hipSuccess;
    void *in(const void *host, size_t bytes)
    {
        void *d = out(bytes);
        if (d && err == hipSuccess) err = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
        return d;
    }
    void *out(size_t bytes)
    {
        void *d = nullptr;
        if (err == hipSuccess) err = hipMalloc(&d, bytes ? bytes : 1);
        if (d) ptrs.push_back(d);
        return d;
    }
    void pull(void *host, const void *d, size_t bytes)
    {
        if (err == hipSuccess) err = hipMemcpy(host, d, bytes, hipMemcpyDeviceToHost);
    }
    void launched()
    {
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
    }
    ~Bufs() { for (void *p : ptrs) (void)hipFree(p); }
};

inline dim3 grid_for(int n) { return dim3((unsigned)((n + 255) / 256)); }

template <int KK, bool INSUP, class T> int run_kernel(int n, int dim, const void *q, void *w, void *dw, void *dwq)
{
    Bufs b;
    const size_t nb = (size_t)n * sizeof(T);
    const T *dq = (const T *)b.in(q, nb);
    T *d0 = (T *)b.out(nb), *d1 = (T *)b.out(nb), *d2 = (T *)b.out(nb);
    if (b.err == hipSuccess) k_kernel<KK, INSUP, T><<<grid_for(n), 256>>>(n, dim, dq, d0, d1, d2);
    b.launched();
    b.pull(w, d0, nb); b.pull(dw, d1, nb); b.pull(dwq, d2, nb);
    return (int)b.err;
}
template <int KK, class T> int run_kernel_i(int insup, int n, int dim, const void *q, void *w, void *dw, void *dwq)
{
    return insup ? run_kernel<KK, true, T>(n, dim, q, w, dw, dwq) : run_kernel<KK, false, T>(n, dim, q, w, dw, dwq);
}
template <class T> int run_kernel_k(int kk, int insup, int n, int dim, const void *q, void *w, void *dw, void *dwq)
{
    switch (kk) {
    case 5: return run_kernel_i<5, T>(insup, n, dim, q, w, dw, dwq);
    case 6: return run_kernel_i<6, T>(insup, n, dim, q, w, dw, dwq);
    case 7: return run_kernel_i<7, T>(insup, n, dim, q, w, dw, dwq);
    case 8: return run_kernel_i<8, T>(insup, n, dim, q, w, dw, dwq);
    case 9: return run_kernel_i<9, T>(insup, n, dim, q, w, dw, dwq);
    case 10: return run_kernel_i<10, T>(insup, n, dim, q, w, dw, dwq);
    }
    return -1;
}

template <int KK, bool UH, class T>
int run_pair(int n, const void *r2, const void *hi, const void *hj, const ProbeArgs &a, void *out)
{
    Bufs b;
    const size_t nb = (size_t)n * sizeof(T);
    const T *d_r2 = (const T *)b.in(r2, nb), *d_hi = (const T *)b.in(hi, nb), *d_hj = (const T *)b.in(hj, nb);
    T *d_out = (T *)b.out(nb * PAIR_OUT);
    if (b.err == hipSuccess) k_pair<KK, UH, T><<<grid_for(n), 256>>>(n, d_r2, d_hi, d_hj, a, d_out);
    b.launched();
    b.pull(out, d_out, nb * PAIR_OUT);
    return (int)b.err;
}
template <int KK, class T>
int run_pair_u(int uh, int n, const void *r2, const void *hi, const void *hj, const ProbeArgs &a, void *out)
{
    return uh ? run_pair<KK, true, T>(n, r2, hi, hj, a, out) : run_pair<KK, false, T>(n, r2, hi, hj, a, out);
}
template <class T>
int run_pair_k(int kk, int uh, int n, const void *r2, const void *hi, const void *hj, const ProbeArgs &a, void *out)
{
    switch (kk) {
    case 5: return run_pair_u<5, T>(uh, n, r2, hi, hj, a, out);
    case 6: return run_pair_u<6, T>(uh, n, r2, hi, hj, a, out);
    case 7: return run_pair_u<7, T>(uh, n, r2, hi, hj, a, out);
    case 8: return run_pair_u<8, T>(uh, n, r2, hi, hj, a, out);
    case 9: return run_pair_u<9, T>(uh, n, r2, hi, hj, a, out);
    case 10: return run_pair_u<10, T>(uh, n, r2, hi, hj, a, out);
    }
    return -1;
}

} // namespace

extern "C" {

// SphKernel<kk>::w/dw/dwq<insup>(q[i], dim), kk = 5..10 (include/sphhip.h enum sph_kernel_kind)
int probe_more_kernel(int kk, int insup, int f32, int n, int dim, const void *q, void *w, void *dw, void *dwq)
{
    if (n <= 0) return -1;
    return f32 ? run_kernel_k<float>(kk, insup, n, dim, q, w, dw, dwq) : run_kernel_k<double>(kk, insup, n, dim, q, w, dw, dwq);
}

// pair_geom<kk, uh>(r2[i], h_i[i], h_j[i]) and pair_w / pair_gradfac / pair_gradh of that geometry;
// out: PAIR_OUT rows of n values (rij rinv hij h1 q fac eps pair_w pair_gradfac pair_gradh).  uh = 1 takes
// HIJ, 1/HIJ, the normalisation and EPS from hu, h1u, facu, epsu like the product's uniform-h launches.
int probe_more_pair(int kk, int uh, int f32, int n, const void *r2, const void *hi, const void *hj, double sigma, int dim,
               double hu, double h1u, double facu, double epsu, void *out)
{
    if (n <= 0) return -1;
    ProbeArgs a;
    a.hu = hu; a.h1u = h1u; a.facu = facu; a.epsu = epsu;
    a.k.sigma = sigma; a.k.deltap = 0.0; a.k.dim = dim;
    return f32 ? run_pair_k<float>(kk, uh, n, r2, hi, hj, a, out) : run_pair_k<double>(kk, uh, n, r2, hi, hj, a, out);
}

} // extern "C"
