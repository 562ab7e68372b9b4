// lo_eigh_f64.hip -- batched symmetric eigendecomposition in fp64 for the exact small-N path (N <= 1024): the dense
// factorisation next to lo_chol_f64.hip.  One workgroup of 256 threads per member, every operand and sum float64,
// fixed-order sums, no atomic, no inter-workgroup communication: a member's result does not depend on the batch it is
// in and repeats bit for bit.
//
// Per member, in the workspace: W [N, N], the full symmetric working copy, and (with vectors) Zt [N, N], the vectors
// TRANSPOSED (eigenvector index outermost).
//   0. scan of the lower triangle: the largest magnitude and a non-finite flag.  The member is scaled by the power of
//      two that brings that magnitude into [0.5, 1), so entries near 1e+-180 neither overflow nor vanish in the norms;
//      the eigenvalues are scaled back (exactly) in the final write.  A non-finite entry ends the member here.
//   1. Householder tridiagonalisation (LAPACK's dsytd2 recurrences, lower form).  Thread j owns column j of the trailing
//      matrix; the rank-2 update of step k - 1 is applied in the same pass that forms the product with the reflector of
//      step k, so the trailing matrix is read and written once per step.  The update a_ij - (v_i w_j + w_i v_j) is
//      evaluated without contraction: W stays symmetric bit for bit, which lets column k be read as row k (coalesced).
//      Reflector k is kept in row k of W right of the diagonal, which no later step reads.  For N <= 128 the rows of a
//      column are split over 256 / TC threads and summed in a fixed order.
//   2. implicit-shift QL (the recurrence and convergence test of lo_eig.hip, at most 30 N sweeps in all as in LAPACK's
//      dsteqr).  Thread 0 runs a sweep's scalar recurrence and leaves its (c, s) sequence in LDS; the threads of the
//      other three waves then apply the whole sequence to their own components of Zt, carrying one value in a register,
//      coalesced, while thread 0 is already in the next sweep's recurrence (it reads d and e only).  Without vectors
//      the same recurrence runs alone: the eigenvalues are the same bits either way.
//   3. back-transformation: a wave keeps 1 to 8 rows of Zt (eigenvectors) in registers, by N, and applies the reflectors
//      H_{N-2} .. H_0 to them, a wave reduction per reflector and row.
//   4. the ascending order (rank by counting, ties by index) and the transposition happen in the final write, through a
//      32 x 33 LDS tile.
// A zero Householder norm gives tau = 0 (H = I); an exact zero off-diagonal passes the convergence test (0 <= 0).
// A failed member (info > 0: 1 = non-finite input, 2 = no convergence) has its outputs filled with NaN.
//
// LDS (doubles, NP = N rounded up to even): d, e, tau [NP each], a scratch region of max(4 NP, 1088) (the pending
// update's (v, w) pairs, the next reflector, the product p; later two buffers of (c, s) pairs; last the transposition
// tile) and 264 for the reductions: 59,456 B at N = 1024, below the 64 KiB a launch gets without opting in.
#include <cfloat>

#include "lo_internal.h"

namespace lo {
namespace {

constexpr int kEighMaxN = LO_EIGH_MAX_N;
constexpr int ET = 32, ETL = 33;    // transposition tile and its row stride
constexpr double kEighEps = 2.3e-16;

struct EighLds {
  int NP, S;
  __host__ __device__ explicit EighLds(int N) : NP((N + 1) & ~1), S(4 * NP > ET * ETL + 32 ? 4 * NP : ET * ETL + 32) {}
  __host__ __device__ size_t bytes() const { return sizeof(double) * (size_t)(3 * NP + S + 264); }
};

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// the same bits in every thread: a butterfly per wave, then the four wave sums in a fixed order
__device__ __forceinline__ double block_sum(double x, double* red) {
  x = wave_sum(x);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ double block_max(double x, double* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = fmax(x, __shfl_xor(x, off, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// One column j of the trailing matrix, rows istart, istart + istep, ...: the pending update is applied and stored, and
// the column's part of (updated trailing matrix) x (next reflector) is returned, summed in row order.
__device__ __forceinline__ double eigh_col_pass(double* __restrict__ Wb, int N, int j, int istart, int istep,
                                                const double2* vw, const double* vn) {
#pragma clang fp contract(off)
  const double2 vwj = vw[j];
  double* col = Wb + j;
  double acc = 0.0;
  int i = istart;
  for (; i + 7 * istep < N; i += 8 * istep) {  // 8 independent loads in flight before the first store
    double a[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] = col[(size_t)(i + u * istep) * N];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int ii = i + u * istep;
      const double2 q = vw[ii];
      const double s = q.x * vwj.y + q.y * vwj.x;  // v_i w_j + w_i v_j: the same bits at (j, i)
      a[u] = a[u] - s;
      col[(size_t)ii * N] = a[u];
      acc = acc + a[u] * vn[ii];
    }
  }
  for (; i < N; i += istep) {
    const double2 q = vw[i];
    const double s = q.x * vwj.y + q.y * vwj.x;
    const double a = col[(size_t)i * N] - s;
    col[(size_t)i * N] = a;
    acc = acc + a * vn[i];
  }
  return acc;
}

// The next sweep of the implicit-shift QL iteration on (d, e) in LDS, one thread: deflates from l upwards, then makes one
// sweep of the block l .. m and leaves its rotations in cs[lo .. m - 1] (CS).  Returns 1 after a sweep, 0 when every
// eigenvalue is found, 2 when the 30 N sweeps are used up.  The recurrence is that of lo_eig.hip; the loads of the next
// step are issued before the stores of this one, and r and 1 / r come from one reciprocal square root with Goldschmidt
// steps (the expansion the compiler uses for sqrt, which yields both) -- the matrix is scaled, f^2 + g^2 cannot overflow,
// and below 1e-290 it goes through hypot.
template <bool CS>
__device__ __forceinline__ int ql_next(double* d, double* e, double2* cs, int N, int& l, int& total, int& m_out,
                                       int& lo_out) {
  l = __builtin_amdgcn_readfirstlane(l);
  while (l < N) {
    int m = l;
    while (m < N - 1) {  // four tests per round of loads; e[N - 1] == 0 passes the test
      double dv[5], evv[4];
#pragma unroll
      for (int u = 0; u < 5; ++u) dv[u] = d[min(m + u, N - 1)];
#pragma unroll
      for (int u = 0; u < 4; ++u) evv[u] = e[min(m + u, N - 1)];
      int hit = -1;
#pragma unroll
      for (int u = 3; u >= 0; --u)
        if (fabs(evv[u]) <= kEighEps * (fabs(dv[u]) + fabs(dv[u + 1]))) hit = u;
      hit = __builtin_amdgcn_readfirstlane(hit);
      if (hit >= 0) {
        m += hit;
        break;
      }
      m += 4;
    }
    m = __builtin_amdgcn_readfirstlane(min(m, N - 1));  // (one thread: the sweep's loop and branches are scalar)
    if (m == l) {
      ++l;
      continue;
    }
    if (total++ >= 30 * N) return 2;
    const double dl = d[l], el = e[l];
    double gg = (d[l + 1] - dl) / (2.0 * el);
    double r = fabs(gg) > 1e150 ? fabs(gg) : sqrt(fma(gg, gg, 1.0));
    gg = d[m] - dl + el / (gg + copysign(r, gg));
    double s = 1.0, c = 1.0, pp = 0.0;
    double en = e[m - 1], dn = d[m - 1], di1 = d[m];
    int i;
    for (i = m - 1; i >= l; --i) {
      const double ei = en, di = dn;
      if (i > l) {
        en = e[i - 1];
        dn = d[i - 1];
      }
      const double f = s * ei, bq = c * ei;
      const double h = fma(f, f, gg * gg);
      double ir;
      if (__builtin_amdgcn_readfirstlane((int)(h < 1e-290))) {
        r = hypot(f, gg);
        if (r == 0.0) {
          e[i + 1] = 0.0;
          d[i + 1] = di1 - pp;
          e[m] = 0.0;
          break;
        }
        ir = 1.0 / r;
      } else {
        const double y = __builtin_amdgcn_rsq(h);
        const double g0 = h * y, h0 = 0.5 * y;
        const double r0 = fma(-h0, g0, 0.5);
        const double g1 = fma(g0, r0, g0), h1 = fma(h0, r0, h0);
        const double g2 = fma(fma(-g1, g1, h), h1, g1);
        r = fma(fma(-g2, g2, h), h1, g2);
        ir = 2.0 * h1;
        ir = fma(ir, fma(-ir, r, 1.0), ir);
      }
      e[i + 1] = r;
      s = f * ir;
      c = gg * ir;
      gg = di1 - pp;
      r = (di - gg) * s + 2.0 * c * bq;
      pp = s * r;
      d[i + 1] = gg + pp;
      gg = c * r - bq;
      if (CS) cs[i] = make_double2(c, s);
      di1 = di;
    }
    if (i >= l) {
      lo_out = i + 1;  // the sweep ended at an underflow: rotations m - 1 .. i + 1 were made
    } else {
      d[l] = dl - pp;
      e[l] = gg;
      e[m] = 0.0;
      lo_out = l;
    }
    m_out = m;
    return 1;
  }
  return 0;
}

// Rotations m - 1 .. lo of a sweep applied to the components t, t + nt, ... of the transposed vectors: rotation i mixes
// rows i and i + 1, the value of row i carried in a register, eight loads in flight.
__device__ __forceinline__ void ql_apply(double* __restrict__ Zb, int N, const double2* cs, int m, int lo, int t, int nt) {
  for (int comp = t; comp < N; comp += nt) {
    double* z = Zb + comp;
    double f = z[(size_t)m * N];
    int i = m - 1;
    for (; i - 7 >= lo; i -= 8) {
      double zi[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) zi[u] = z[(size_t)(i - u) * N];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const double2 q = cs[i - u];
        z[(size_t)(i - u + 1) * N] = fma(q.y, zi[u], q.x * f);
        f = fma(q.x, zi[u], -(q.y * f));
      }
    }
    for (; i >= lo; --i) {
      const double2 q = cs[i];
      const double zi = z[(size_t)i * N];
      z[(size_t)(i + 1) * N] = fma(q.y, zi, q.x * f);
      f = fma(q.x, zi, -(q.y * f));
    }
    z[(size_t)lo * N] = f;
  }
}

// Back-transformation of R rows of Zt (R eigenvectors) per wave, each row's NQ chunks of 64 components in registers:
// H_k = I - tau_k v_k v_k^T for k = N - 2 .. 0, v_k in row k of W right of the diagonal.  One butterfly per row and
// reflector, the R butterflies interleaved; the reflector of step k - 1 is requested before the sums of step k.
template <int NQ, int R>
__device__ __forceinline__ void eigh_back_rows(double* __restrict__ Zb, const double* __restrict__ Wb, const double* tau,
                                               int N, int wave, int lane) {
  for (int jb = R * wave; jb < N; jb += 4 * R) {
    double r[R][NQ], vv[NQ], vx[NQ];
#pragma unroll
    for (int t = 0; t < R; ++t)
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int i = lane + 64 * q;
        r[t][q] = (i < N && jb + t < N) ? Zb[(size_t)(jb + t) * N + i] : 0.0;
      }
#pragma unroll
    for (int q = 0; q < NQ; ++q) vv[q] = (N >= 2) ? Wb[(size_t)(N - 2) * N + min(lane + 64 * q, N - 1)] : 0.0;
    for (int k = N - 2; k >= 0; --k) {
      const double tk = tau[k];
      const double* vk = Wb + (size_t)max(k - 1, 0) * N;
#pragma unroll
      for (int q = 0; q < NQ; ++q) vx[q] = vk[min(lane + 64 * q, N - 1)];
      if (tk != 0.0) {
        double s[R];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const int i = lane + 64 * q;
          vv[q] = (i > k && i < N) ? vv[q] : 0.0;
        }
#pragma unroll
        for (int t = 0; t < R; ++t) {
          s[t] = 0.0;
#pragma unroll
          for (int q = 0; q < NQ; ++q) s[t] = fma(vv[q], r[t][q], s[t]);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
#pragma unroll
          for (int t = 0; t < R; ++t) s[t] += __shfl_xor(s[t], off, 64);
#pragma unroll
        for (int t = 0; t < R; ++t) {
          const double st = s[t] * tk;
#pragma unroll
          for (int q = 0; q < NQ; ++q) r[t][q] = fma(-st, vv[q], r[t][q]);
        }
      }
#pragma unroll
      for (int q = 0; q < NQ; ++q) vv[q] = vx[q];
    }
#pragma unroll
    for (int t = 0; t < R; ++t)
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int i = lane + 64 * q;
        if (i < N && jb + t < N) Zb[(size_t)(jb + t) * N + i] = r[t][q];
      }
  }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_eigh_f64(const double* __restrict__ A, double* __restrict__ W,
                                                       double* __restrict__ Zt, double* __restrict__ evals,
                                                       double* __restrict__ evecs, int* __restrict__ info, int N,
                                                       int tc_log2) {
  extern __shared__ __attribute__((aligned(16))) double smd[];
  __shared__ int ctl[8];
  const EighLds L(N);
  double* d = smd;
  double* e = d + L.NP;
  double* tau = e + L.NP;
  double* scr = tau + L.NP;
  double2* vw = reinterpret_cast<double2*>(scr);  // [NP] (v_i, w_i) of the pending rank-2 update
  double* vn = scr + 2 * L.NP;                    // [NP] the column of step k, then its reflector
  double* p = scr + 3 * L.NP;                     // [NP] trailing matrix x reflector
  double* red = scr + L.S;                        // [264]
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const double* Ab = A + (size_t)b * N * N;
  double* Wb = W + (size_t)b * N * N;
  double* Zb = VEC ? Zt + (size_t)b * N * N : nullptr;
  double* ev = evals + (size_t)b * N;
  double* eo = VEC ? evecs + (size_t)b * N * N : nullptr;
  const int NN = N * N;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);

  // ---- 0. largest magnitude, non-finite entries
  double amax = 0.0, bad = 0.0;
  for (int idx = tid; idx < NN; idx += kThreads) {
    const int r = idx / N, c = idx - r * N;
    if (c <= r) {
      const double x = fabs(Ab[idx]);
      if (!(x <= DBL_MAX)) bad = 1.0;
      amax = fmax(amax, x);
    }
  }
  bad = block_max(bad, red);
  amax = block_max(amax, red);
  int fail = bad > 0.0 ? 1 : 0;
  int ex = 0;
  if (!fail && amax > 0.0) {
    (void)frexp(amax, &ex);
    ex = max(-1020, min(1020, ex));
  }
  if (!fail) {
    const double sigma = ldexp(1.0, -ex);
    for (int idx = tid; idx < NN; idx += kThreads) {
      const int r = idx / N, c = idx - r * N;
      Wb[idx] = sigma * (c <= r ? Ab[idx] : Ab[(size_t)c * N + r]);
    }
    for (int i = tid; i < L.NP; i += kThreads) {
      vw[i] = make_double2(0.0, 0.0);
      e[i] = 0.0;
      tau[i] = 0.0;
    }
    __syncthreads();

    // ---- 1. tridiagonalisation
    const int TC = 1 << tc_log2, RG = kThreads >> tc_log2, cc = tid & (TC - 1), g = tid >> tc_log2;
    for (int k = 0; k + 1 < N; ++k) {
      const double* rowk = Wb + (size_t)k * N;
      const double2 vwk = vw[k];
      double ss = 0.0;
      {
#pragma clang fp contract(off)
        for (int i = k + tid; i < N; i += kThreads) {
          const double2 q = vw[i];
          const double x = rowk[i] - (q.x * vwk.y + q.y * vwk.x);
          vn[i] = x;
          if (i >= k + 2) ss = ss + x * x;
        }
      }
      ss = block_sum(ss, red);  // (its barriers also publish vn)
      const double alpha = vn[k + 1], dk = vn[k];
      double tk = 0.0, ek = alpha, scal = 0.0;
      if (ss > 0.0) {
        const double beta = -copysign(sqrt(alpha * alpha + ss), alpha);
        tk = (beta - alpha) / beta;
        scal = 1.0 / (alpha - beta);
        ek = beta;
      }
      __syncthreads();  // every thread has read vn[k], vn[k + 1]
      for (int i = k + 1 + tid; i < N; i += kThreads) {
        const double v = (i == k + 1) ? 1.0 : vn[i] * scal;
        vn[i] = v;
        if (VEC) Wb[(size_t)k * N + i] = v;
      }
      if (tid == 0) {
        d[k] = dk;
        e[k] = ek;
        tau[k] = tk;
      }
      __syncthreads();
      const int j0 = k + 1;
      if (RG == 1) {
        for (int j = j0 + tid; j < N; j += kThreads) p[j] = eigh_col_pass(Wb, N, j, j0, 1, vw, vn);
      } else {
        const int j = j0 + cc;
        red[tid] = (j < N) ? eigh_col_pass(Wb, N, j, j0 + g, RG, vw, vn) : 0.0;
        __syncthreads();
        if (g == 0 && j < N) {
          double s = 0.0;
          for (int gg = 0; gg < RG; ++gg) s += red[gg * TC + cc];
          p[j] = s;
        }
      }
      __syncthreads();
      double dot = 0.0;
      for (int j = j0 + tid; j < N; j += kThreads) dot = fma(p[j], vn[j], dot);
      dot = block_sum(dot, red);
      const double a2 = -0.5 * tk * tk * dot;
      for (int j = j0 + tid; j < N; j += kThreads) vw[j] = make_double2(vn[j], fma(tk, p[j], a2 * vn[j]));
      __syncthreads();
    }
    if (tid == 0) {
      const double2 q = vw[N - 1];
      d[N - 1] = Wb[(size_t)(N - 1) * N + N - 1] - 2.0 * (q.x * q.y);
      e[N - 1] = 0.0;
    }
    if (VEC)
      for (int idx = tid; idx < NN; idx += kThreads) {
        const int r = idx / N, c = idx - r * N;
        Zb[idx] = (r == c) ? 1.0 : 0.0;
      }
    __syncthreads();

    // ---- 2. implicit-shift QL
    double2* csb = reinterpret_cast<double2*>(scr);  // two buffers [NP] of (c, s) per rotation
    if (!VEC) {
      if (tid == 0) {
        int l = 0, total = 0, m, lo, st;
        while ((st = ql_next<false>(d, e, csb, N, l, total, m, lo)) == 1) {
        }
        ctl[0] = st;
      }
      __syncthreads();
      if (ctl[0] == 2) fail = 2;
    } else {
      // Thread 0 runs the recurrence of sweep t + 1 while waves 1 .. 3 apply the rotations of sweep t (the recurrence
      // reads d and e only): one barrier per sweep, (c, s) and the control words double-buffered.
      int l = 0, total = 0;  // thread 0
      int buf = 0, have_prev = 0, pm = 0, plo = 0;
      for (;;) {
        if (wave == 0) {
          if (tid == 0) {
            int m, lo;
            const int st = ql_next<true>(d, e, csb + buf * L.NP, N, l, total, m, lo);
            ctl[4 * buf] = st;
            ctl[4 * buf + 1] = m;
            ctl[4 * buf + 2] = lo;
          }
        } else if (have_prev) {
          ql_apply(Zb, N, csb + (buf ^ 1) * L.NP, pm, plo, tid - 64, kThreads - 64);
        }
        __syncthreads();
        const int st = ctl[4 * buf];
        pm = ctl[4 * buf + 1];
        plo = ctl[4 * buf + 2];
        if (st != 1) {  // finished (the last sweep was applied in this round) or failed
          if (st == 2) fail = 2;
          break;
        }
        have_prev = 1;
        buf ^= 1;
      }
      __syncthreads();
    }
  }

  if (fail) {  // (uniform) the member's outputs are NaN, the others are not touched
    for (int i = tid; i < N; i += kThreads) ev[i] = qnan;
    if (VEC)
      for (int idx = tid; idx < NN; idx += kThreads) eo[idx] = qnan;
    if (tid == 0) info[b] = fail;
    return;
  }

  // ---- 3. back-transformation: rows of Zt (eigenvectors) in registers, reflectors N - 2 .. 0
  if (VEC) {
    if (N <= 64) eigh_back_rows<1, 8>(Zb, Wb, tau, N, wave, lane);
    else if (N <= 128) eigh_back_rows<2, 8>(Zb, Wb, tau, N, wave, lane);
    else if (N <= 256) eigh_back_rows<4, 8>(Zb, Wb, tau, N, wave, lane);
    else if (N <= 512) eigh_back_rows<8, 4>(Zb, Wb, tau, N, wave, lane);
    else eigh_back_rows<16, 1>(Zb, Wb, tau, N, wave, lane);
    __syncthreads();
  }

  // ---- 4. ascending order and the final (transposed) write
  int* src = reinterpret_cast<int*>(e);  // [N] src[rank] = index
  for (int i = tid; i < N; i += kThreads) {
    const double di = d[i];
    int rank = 0;
    for (int j = 0; j < N; ++j) {
      const double dj = d[j];
      rank += (dj < di || (dj == di && j < i)) ? 1 : 0;
    }
    ev[rank] = ldexp(di, ex);
    src[rank] = i;
  }
  if (tid == 0) info[b] = 0;
  if (VEC) {
    __syncthreads();
    double* tile = scr;  // [32][33]
    const int tx = tid & 31, ty = tid >> 5;
    for (int r0 = 0; r0 < N; r0 += ET) {
      for (int k0 = 0; k0 < N; k0 += ET) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int yy = ty + 8 * u, r = r0 + yy, k = k0 + tx;
          if (r < N && k < N) tile[yy * ETL + tx] = Zb[(size_t)src[r] * N + k];
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int yy = ty + 8 * u, k = k0 + yy, r = r0 + tx;
          if (r < N && k < N) eo[(size_t)k * N + r] = tile[tx * ETL + yy];
        }
        __syncthreads();
      }
    }
  }
}

// the workspace of lo_eigh_f64: the working copy [B, N, N] and, with vectors, the transposed vectors [B, N, N]
constexpr size_t kEighTail = 512;  // what the sizer reports beyond the layout
struct EighBufs { double* W; double* Zt; };
EighBufs eigh_layout(Arena& ar, int64_t B, int64_t N, bool vec) {
  EighBufs r;
  r.W = ar.take<double>((size_t)B * N * N);
  r.Zt = vec ? ar.take<double>((size_t)B * N * N) : nullptr;
  return r;
}

template <bool VEC>
int eigh_launch(const double* A, const EighBufs& bufs, double* evals, double* evecs, int* info, int64_t B, int N,
                hipStream_t st) {
  const EighLds L(N);
  const size_t lds = L.bytes();
  if (lds > 64 * 1024)  // (not reached at N <= 1024; the opt-in belongs to the current device: set it per launch)
    LO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_eigh_f64<VEC>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  int tc_log2 = 8;  // threads across the columns of the trailing matrix; the other 256 / TC split a column's rows
  if (N <= 128) {
    tc_log2 = 5;
    while ((1 << tc_log2) < N) ++tc_log2;
  }
  LO_PROF_BEGIN(VEC ? "eigh_f64" : "eigvalsh_f64", st);
  hipLaunchKernelGGL(k_eigh_f64<VEC>, dim3((unsigned)B), dim3(kThreads), lds, st, A, bufs.W, bufs.Zt, evals, evecs,
                     info, N, tc_log2);
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

}  // namespace
}  // namespace lo

using namespace lo;

extern "C" {

size_t lo_eigh_f64_workspace_bytes(int64_t B, int64_t N, int32_t want_vectors) {
  if (B < 1 || B > 0x7fffffff || N < 1 || N > kEighMaxN) return 0;
  return measured(kEighTail, [&](Arena& ar) { eigh_layout(ar, B, N, want_vectors != 0); });
}

int lo_eigh_f64(const double* A, double* evals, double* evecs, int32_t* info, int64_t B, int64_t N,
                int32_t want_vectors, void* ws, size_t ws_bytes, void* stream) {
  if (!A || !evals || !info || (want_vectors && !evecs) || B < 0 || N < 1) return LO_ERR_BADARG;
  if (N > kEighMaxN || B > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  if (B == 0) return LO_OK;
  Arena ar(ws, ws_bytes, kEighTail);
  const EighBufs bufs = eigh_layout(ar, B, N, want_vectors != 0);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (want_vectors) return eigh_launch<true>(A, bufs, evals, evecs, info, B, (int)N, st);
  return eigh_launch<false>(A, bufs, evals, nullptr, info, B, (int)N, st);
}

}  // extern "C"
