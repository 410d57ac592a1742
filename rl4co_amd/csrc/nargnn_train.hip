// nargnn_train.hip — the GNN stack of DeepACO's heatmap encoder in TRAIN mode and its backward (the reference's
// models/nn/graph/gnn.py:45-61 with batch norms on batch statistics) for gfx950, fp32, on two graphs: the regular k-nearest
// graph of TSP (rl4co_nargnn_train_*) and the depot graph of CVRP, OP and PCTSP (rl4co_nargnn_depot_train_*). The math and
// the C contract are in include/rl4co_amd.h (rl4co_nargnn_train_args, rl4co_nargnn_depot_train_args); the MFMA tile product
// and its operand convention are nargnn_shared.h's. What a graph is to these kernels -- the edge rows per instance, a row's
// two ends, a node's outgoing rows and its degree -- is stated once per graph (`Regular`, `Depot` below); k_check, the two
// edge MFMA passes and the two node passes are templated on it, everything else does not know the graph.
//
// Nothing stays on chip across a layer: a batch norm needs every row of the batch before any row can go on. The work is
// split by ROWS (16-row tiles of the flat [B N] node rows and [B N K] edge rows -- [B (N - 1)(K + 2)] on the depot graph --
// rows of 64 floats), never by instance, and every batch-wide reduction crosses a launch boundary: a pass writes one
// partial per workgroup, a one-workgroup finalize launch combines the partials in ascending order, the next pass applies
// the result. No grid barrier, no spin, no floating-point atomic; every sum has a fixed order, so every output is
// bit-identical run to run.
//
// A workgroup is four waves; rows R are cut into P(R) = min(ceil(R / 64), 1024) workgroups and each of the 4 P waves takes
// a contiguous run of ceil(ceil(R / 16) / 4 P) tiles. Forward, per layer (6 launches):
//   lin_fwd<node>   x1, x2, x3, x4 = v_lin1 .. v_lin4 (x0)                       MFMA, grid.y = matrix; x2 is saved
//   vert_pre        pre_v[i] = x1[i] + (sum_k sigmoid(w0[i,k]) x2[j]) / deg(i)    wave = node, lane = channel
//   lin_fwd<edge>   pre_e[e] = (e_lin(w0)[e] + x3[i]) + x4[j]                      MFMA
//   row_stats       per workgroup (count, mean, M2) of pre_v and of pre_e, the mean and the M2 about it taken in two
//                   sweeps of the wave's own rows (the second one hits the cache), summed in float64
//   stats_finalize  Chan's combination of the partials (float64) -> mu, r = 1 / sqrt(var + eps), var
//   apply           x = x0 + silu(gamma (pre_v - mu) r + beta), w alike; the last layer writes x_out / w_out
// Backward, per layer from the last (10 launches); gx, gw are the gradients of the layer's outputs:
//   bwd_reduce      per workgroup sum gy, sum gy u^ on both sides, gy = g silu'(y)
//   bwd_finalize    d beta, d gamma and the two means
//   bwd_gu          gu = gamma r (gy - mean gy - u^ mean(gy u^)) -> gu_v (node plane 0) and gu_e
//   lin_bwd<edge>   gw0 = gw + gu_e W_e + gu_v[i] x2[j] s (1 - s) / deg(i); partials of dW_e = gu_e^T w0 and db_e  MFMA
//   node_bwd        gx2[j], gx4[j] over j's incoming edges (the CSR, ascending), gx3[i] over i's own rows      wave = node
//   lin_bwd<node>   four launches, m = 1 .. 4: gx0 (+)= gx_m W_m; partials of dW_m = gx_m^T x0 and db_m              MFMA
//   dw_finalize     the five matrices' partials, ascending
// The running gradients gx and gw live in one buffer each: lin_bwd reads and writes an element in the same lane.
// The first launch of either call checks `neighbors` and the CSR and raises a flag in the workspace head; every other kernel
// returns at once when it is set, so nothing is read through a bad index.
// The depot's sums (its mean, its gx3 and its incoming sums are N - 1 terms long, every other node's K + 1 or so) are taken
// as eight interleaved partial sums, term t into partial t mod 8, combined as ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)): eight
// loads in flight instead of one, and an order that depends on nothing but the node.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "nargnn_shared.h"
#include "rl4co_math.h"

namespace {

using namespace rl4co::nargnn;

constexpr int kT = 256;          // threads of a workgroup
constexpr int kW = kT / 64;      // waves
constexpr int kMaxGroups = 1024;
constexpr int kPartDw = kD * kD + kD;  // one workgroup's weight-gradient partial: dW [64][64], db [64]
constexpr int kHead = 64;        // workspace head (floats): word 0 is the bad-input flag

__device__ inline float sigm(float x) { return 1.0f / (1.0f + rl4co_expf(-x)); }
__device__ inline float silu(float x) { return x / (1.0f + rl4co_expf(-x)); }

// ---- the workspace (floats) -------------------------------------------------------------------------------------------------
inline int groups_of(int64_t rows) { return (int)std::min<int64_t>((rows + 63) / 64, kMaxGroups); }
inline int tiles_per_wave(int64_t rows, int P) {
  const int64_t tiles = (rows + 15) / 16, waves = (int64_t)kW * P;
  return (int)((tiles + waves - 1) / waves);
}
struct Layout {
  int64_t nv, ne;  // floats of a node plane and of an edge plane
  int Pv, Pe;
  int64_t xs, ws, pv, x2, pe, t, gx, gue, gw, part, dw, means, total;
};
inline Layout layout(int64_t n_v, int64_t n_e, int64_t L) {
  Layout y;
  y.nv = n_v * kD;
  y.ne = n_e * kD;
  y.Pv = groups_of(n_v);
  y.Pe = groups_of(n_e);
  const int64_t Lm = L > 1 ? L - 1 : 0;
  int64_t at = kHead;
  const auto take = [&](int64_t n) { const int64_t o = at; at += n; return o; };
  y.xs = take(Lm * y.nv);
  y.ws = take(Lm * y.ne);
  y.pv = take(L * y.nv);
  y.x2 = take(L * y.nv);
  y.pe = take(L * y.ne);
  y.t = take(4 * y.nv);
  y.gx = take(y.nv);
  y.gue = take(y.ne);
  y.gw = take(y.ne);
  y.part = take((int64_t)192 * (y.Pv + y.Pe));
  y.dw = take((int64_t)kPartDw * (4 * y.Pv + y.Pe));
  y.means = take(512);
  y.total = at;
  return y;
}

// ---- the two graphs -------------------------------------------------------------------------------------------------------------
// A graph says: the edge rows and the entries of `neighbors` per instance, the smallest neighbour index, the two ends of an
// edge row and the out-degree of its source (`ends`), a node (`node`), that node's t-th outgoing row and its target (`out`),
// and the source of one of its INCOMING rows with that source's out-degree (`source`). Nothing is stored: all are closed
// forms of (row, neighbors).
struct Regular {  // TSP: node i's K rows are i K .. i K + K - 1, row e is e / K -> neighbors[e]
  static constexpr bool kDepot = false;
  static constexpr int kMinN = 2, kFirst = 0;
  int N, K;
  __host__ __device__ Regular(int n, int k) : N(n), K(k) {}
  __host__ __device__ int64_t rows() const { return (int64_t)N * K; }
  __host__ __device__ int64_t lists() const { return (int64_t)N * K; }
  struct Node {
    int64_t v, base;
    int deg;
    bool depot;
  };
  __device__ void ends(int64_t e, const int32_t* nbr, int64_t& i, int64_t& j, float& deg) const {
    i = e / K;
    j = (i / N) * N + nbr[e];
    deg = (float)K;
  }
  __device__ Node node(int64_t v) const { return Node{v, (v / N) * N, K, false}; }
  __device__ void out(const Node& nd, int t, const int32_t* nbr, int64_t& e, int64_t& j) const {
    e = nd.v * K + t;
    j = nd.base + nbr[e];
  }
  __device__ void source(const Node&, int64_t e, int64_t& i, float& deg) const {
    i = e / K;
    deg = (float)K;
  }
};
// CVRP, OP, PCTSP (CVRPEdgeEmbedding): C = N - 1 customers, E = C (K + 2) rows per instance in the reference's order:
// [0, C K) the kNN rows by source, row (i - 1) K + k is i -> neighbors[i - 1, k]; [C K, C K + C) i -> 0; then 0 -> i.
// A customer's out-degree is K + 1 (its K rows and its i -> 0 row), the depot's is C.
struct Depot {
  static constexpr bool kDepot = true;
  static constexpr int kMinN = 3, kFirst = 1;  // the depot is nobody's kNN neighbour
  int N, K, C, CK, E;
  __host__ __device__ Depot(int n, int k) : N(n), K(k), C(n - 1), CK((n - 1) * k), E((n - 1) * (k + 2)) {}
  __host__ __device__ int64_t rows() const { return E; }
  __host__ __device__ int64_t lists() const { return CK; }
  struct Node {
    int64_t base, row0, list0;  // the instance's first node, first edge row and first entry of `neighbors`
    int li, deg;
    bool depot;
  };
  __device__ void ends(int64_t e, const int32_t* nbr, int64_t& i, int64_t& j, float& deg) const {
    const int b = (int)e / E, r = (int)e - b * E;  // (e < 2^24)
    const int64_t base = (int64_t)b * N;
    if (r < CK) {
      i = base + 1 + r / K;
      j = base + nbr[(int64_t)b * CK + r];
      deg = (float)(K + 1);
    } else if (r < CK + C) {
      i = base + 1 + (r - CK);
      j = base;
      deg = (float)(K + 1);
    } else {
      i = base;
      j = base + 1 + (r - CK - C);
      deg = (float)C;
    }
  }
  __device__ Node node(int64_t v) const {
    const int64_t b = v / N;
    const int li = (int)(v - b * N);
    return Node{b * N, b * E, b * CK, li, li == 0 ? C : K + 1, li == 0};
  }
  __device__ void out(const Node& nd, int t, const int32_t* nbr, int64_t& e, int64_t& j) const {
    if (nd.depot) {
      e = nd.row0 + CK + C + t;
      j = nd.base + 1 + t;
    } else if (t < K) {
      const int r = (nd.li - 1) * K + t;
      e = nd.row0 + r;
      j = nd.base + nbr[nd.list0 + r];
    } else {
      e = nd.row0 + CK + (nd.li - 1);
      j = nd.base;
    }
  }
  __device__ void source(const Node& nd, int64_t e, int64_t& i, float& deg) const {  // e: a row of nd's instance
    const int r = (int)(e - nd.row0);
    i = r < CK ? nd.base + 1 + r / K : r < CK + C ? nd.base + 1 + (r - CK) : nd.base;
    deg = r < CK + C ? (float)(K + 1) : (float)C;
  }
};

// term(0) + .. + term(n - 1) as eight interleaved partial sums (the depot's long sums)
template <class T, class F>
__device__ inline T sum8(int n, F term) {
  T p[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) p[q] = T{};
  int t = 0;
  for (; t + 8 <= n; t += 8) {
#pragma unroll
    for (int q = 0; q < 8; ++q) p[q] += term(t + q);
  }
#pragma unroll
  for (int q = 0; q < 7; ++q)
    if (t + q < n) p[q] += term(t + q);
  return ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
}
// the same sum for any node of graph G: in order, the depot's by sum8
template <class T, class G, class F>
__device__ inline T node_sum(bool depot, int n, F term) {
  if (G::kDepot && depot) return sum8<T>(n, term);
  T s{};
  for (int t = 0; t < n; ++t) s += term(t);
  return s;
}
// a node's two incoming sums, taken in one walk of its rows
struct Incoming {
  double g4;
  float g2;
  __device__ Incoming& operator+=(const Incoming& o) {
    g4 += o.g4;
    g2 += o.g2;
    return *this;
  }
  friend __device__ Incoming operator+(Incoming a, const Incoming& o) { return a += o; }
};

// ---- the check ----------------------------------------------------------------------------------------------------------------
struct CheckArgs {
  const int32_t *nbr, *ptr, *src;
  int64_t n_v, n_e, n_l;  // node rows, edge rows, entries of nbr
  int N, K;
  int* bad;
  int32_t* err;
};
template <class G>
__global__ void __launch_bounds__(kT) k_check(const CheckArgs a) {
  const G gr(a.N, a.K);
  const int64_t tid = (int64_t)blockIdx.x * kT + threadIdx.x, stride = (int64_t)gridDim.x * kT;
  const int lane = threadIdx.x & 63;
  bool bad = false;
  for (int64_t e = tid; e < a.n_l; e += stride) {
    const int v = a.nbr[e];
    bad |= v < G::kFirst || v >= a.N;
  }
  if (tid == 0) bad |= a.ptr[0] != 0 || (int64_t)a.ptr[a.n_v] != a.n_e;
  for (int64_t j = tid >> 6; j < a.n_v; j += stride >> 6) {
    const int64_t p0 = a.ptr[j], p1 = a.ptr[j + 1];
    if (p0 < 0 || p1 > a.n_e || p0 > p1) {
      bad = true;
      continue;
    }
    for (int64_t p = p0 + lane; p < p1; p += 64) {
      const int64_t e = a.src[p];
      if (e < 0 || e >= a.n_e) {
        bad = true;
        continue;
      }
      int64_t i, jj;  // (a bad neighbour gives a wrong jj and nothing else: the loop above has raised the flag for it)
      float deg;
      gr.ends(e, a.nbr, i, jj, deg);
      if (jj != j) bad = true;
      if (p > p0 && (int64_t)a.src[p - 1] >= e) bad = true;
    }
  }
  if (bad) {
    atomicOr(a.bad, 1);
    atomicOr(a.err, RL4CO_EBIT_TOUR_INDEX);
  }
}

// ---- the MFMA passes ------------------------------------------------------------------------------------------------------------
// the transposed fragments: gemm_tile with them gives (16 rows) . W for W row-major [out][in]: fragment [ct][j] of lane
// (c, g) is W[16 j + 4 g ..][16 ct + c]
__device__ inline void load_wfrags_t(f32x4 (&wf)[4][4], const float* W, int lane) {
  const int c = lane & 15, g = lane >> 4;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int s = 0; s < 4; ++s) wf[ct][j][s] = W[(16 * j + 4 * g + s) * kD + 16 * ct + c];
}

struct LinFwdArgs {
  const int* bad;
  const float* X;   // [rows][64]
  const float* W;   // [M][64][64]
  const float* b;   // [M][64]
  float* Y[4];      // per matrix
  int64_t rows;
  int tpw;
  const float *X3, *X4;  // edge: the node planes added to the product
  const int32_t* nbr;
  int N, K;
};
template <bool EDGE, class G>
__global__ void __launch_bounds__(kT) k_lin_fwd(const LinFwdArgs a) {
  if (*a.bad) return;
  const G gr(a.N, a.K);
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int m = EDGE ? 0 : blockIdx.y;
  const int64_t wg = (int64_t)blockIdx.x * kW + (threadIdx.x >> 6);
  f32x4 wf[4][4];
  load_wfrags(wf, a.W + m * kD * kD, lane);
  float bcol[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) bcol[ct] = a.b[m * kD + 16 * ct + c];
  float* Y = a.Y[m];
  const int64_t tiles = (a.rows + 15) >> 4;
  const int64_t t1 = min(tiles, (wg + 1) * a.tpw);
  for (int64_t t = wg * a.tpw; t < t1; ++t) {
    const int64_t row = min(16 * t + c, a.rows - 1);  // rows past the end repeat the last one and are not stored
    f32x4 acc[4];
    gemm_tile(acc, wf, a.X + row * kD + 4 * g);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t n = 16 * t + 4 * g + r;
      if (n < a.rows) {
        if constexpr (EDGE) {
          int64_t i, j;
          float deg;
          gr.ends(n, a.nbr, i, j, deg);
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) {
            const int col = 16 * ct + c;
            Y[n * kD + col] = ((acc[ct][r] + bcol[ct]) + a.X3[i * kD + col]) + a.X4[j * kD + col];
          }
        } else {
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) Y[n * kD + 16 * ct + c] = acc[ct][r] + bcol[ct];
        }
      }
    }
  }
}

struct LinBwdArgs {
  const int* bad;
  const float* GU;   // [rows][64]: the gradient of the linear's output
  const float* X;    // [rows][64]: the linear's input
  const float* W;    // [64][64]
  const float* ADD;  // [rows][64]; may be OUT (an element is read and written by one lane)
  float* OUT;        // [rows][64] = ADD + GU . W (+ the edge term)
  float* part;       // [P][kPartDw]
  int64_t rows;
  int tpw;
  const float *GUV, *X2;  // edge: gu_v, x2
  const int32_t* nbr;
  int N, K;
};
template <bool EDGE, class G>
__global__ void __launch_bounds__(kT) k_lin_bwd(const LinBwdArgs a) {
  __shared__ float sdw[kD * kD];
  __shared__ double sdb[kW][4][kD];
  if (*a.bad) return;
  const G gr(a.N, a.K);
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int w = threadIdx.x >> 6;
  const int64_t wg = (int64_t)blockIdx.x * kW + w;
  f32x4 dw[4][4];
  double db[4];  // (a bias ahead of a batch norm has a zero gradient: what is left is this sum's rounding)
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    db[mt] = 0.0;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) dw[mt][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }
  {
    f32x4 wf[4][4];
    load_wfrags_t(wf, a.W, lane);
    const int64_t tiles = (a.rows + 15) >> 4;
    const int64_t t1 = min(tiles, (wg + 1) * a.tpw);
    for (int64_t t = wg * a.tpw; t < t1; ++t) {
      const int64_t row = min(16 * t + c, a.rows - 1);
      f32x4 acc[4];
      gemm_tile(acc, wf, a.GU + row * kD + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t n = 16 * t + 4 * g + r;
        if (n < a.rows) {
          int64_t i = 0, j = 0;
          float count = 1.0f;  // the out-degree of the row's source
          if constexpr (EDGE) gr.ends(n, a.nbr, i, j, count);
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) {
            const int col = 16 * ct + c;
            float v = a.ADD[n * kD + col] + acc[ct][r];
            if constexpr (EDGE) {
              const float s = sigm(a.X[n * kD + col]);
              v += ((a.GUV[i * kD + col] * a.X2[j * kD + col]) * (s * (1.0f - s))) / count;
            }
            a.OUT[n * kD + col] = v;
          }
        }
      }
      // dW[n][k] += sum over the tile's rows of GU[row][n] X[row][k]: the rows are the MFMA's k dimension, four a step
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int64_t rr = 16 * t + 4 * s + g;
        const bool ok = rr < a.rows;
        const int64_t at = (ok ? rr : 0) * kD + c;
        float av[4], bv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          av[q] = ok ? a.GU[at + 16 * q] : 0.0f;
          bv[q] = ok ? a.X[at + 16 * q] : 0.0f;
          db[q] += (double)av[q];
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) dw[mt][nt] = mfma4(av[mt], bv[nt], dw[mt][nt]);
      }
    }
  }
  // the four waves' sums, wave 0 first
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) sdb[w][g][16 * mt + c] = db[mt];
  for (int turn = 0; turn < kW; ++turn) {
    if (w == turn) {
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int at = (16 * mt + 4 * g + r) * kD + 16 * nt + c;
            sdw[at] = turn == 0 ? dw[mt][nt][r] : sdw[at] + dw[mt][nt][r];
          }
    }
    __syncthreads();
  }
  float* part = a.part + (int64_t)blockIdx.x * kPartDw;
  for (int at = threadIdx.x; at < kD * kD; at += kT) part[at] = sdw[at];
  if (threadIdx.x < kD) {
    double s = 0.0;
    for (int ww = 0; ww < kW; ++ww)
      for (int gg = 0; gg < 4; ++gg) s += sdb[ww][gg][threadIdx.x];
    part[kD * kD + threadIdx.x] = (float)s;
  }
}

struct DwFinalArgs {
  const int* bad;
  const float* part;  // the five matrices' partials: 4 x [Pv][kPartDw], then [Pe][kPartDw]
  int Pv, Pe;
  float *gw, *gb;  // this layer's [5][64][64], [5][64]
};
__global__ void __launch_bounds__(kT) k_dw_finalize(const DwFinalArgs a) {
  if (*a.bad) return;
  const int at = blockIdx.x * kT + threadIdx.x, m = blockIdx.y;
  if (at >= kPartDw) return;
  const float* part = a.part + (int64_t)m * a.Pv * kPartDw + at;
  const int P = m < 4 ? a.Pv : a.Pe;
  double s = 0.0;
  for (int p = 0; p < P; ++p) s += (double)part[(int64_t)p * kPartDw];
  if (at < kD * kD) a.gw[m * kD * kD + at] = (float)s;
  // a bias directly ahead of a batch norm (v_lin1, v_lin3, v_lin4, e_lin: every linear but v_lin2) shifts a channel by a
  // constant, which the batch mean takes out again: its gradient is zero in exact arithmetic, and the sum above holds
  // nothing but the rounding of its terms. The exact value is written.
  else a.gb[m * kD + at - kD * kD] = m == 1 ? (float)s : 0.0f;
}

// ---- the node passes (wave = node, lane = channel) ------------------------------------------------------------------------------
struct NodeArgs {
  const int* bad;
  const int32_t *nbr, *ptr, *src;
  const float *W0, *X1, *X2;  // forward
  float* PV;
  const float *GUE, *GUV;  // backward
  float *G2, *G3, *G4;
  int64_t n_v;
  int rpw, N, K;
};
template <class G>
__global__ void __launch_bounds__(kT) k_vert_pre(const NodeArgs a) {
  if (*a.bad) return;
  const G gr(a.N, a.K);
  const int lane = threadIdx.x & 63;
  const int64_t wg = (int64_t)blockIdx.x * kW + (threadIdx.x >> 6);
  const int64_t i1 = min(a.n_v, (wg + 1) * a.rpw);
  for (int64_t i = wg * a.rpw; i < i1; ++i) {
    const typename G::Node nd = gr.node(i);
    const float s = node_sum<float, G>(nd.depot, nd.deg, [&](int t) {
      int64_t e, j;
      gr.out(nd, t, a.nbr, e, j);
      return sigm(a.W0[e * kD + lane]) * a.X2[j * kD + lane];
    });
    a.PV[i * kD + lane] = a.X1[i * kD + lane] + s / (float)nd.deg;
  }
}
template <class G>
__global__ void __launch_bounds__(kT) k_node_bwd(const NodeArgs a) {
  if (*a.bad) return;
  const G gr(a.N, a.K);
  const int lane = threadIdx.x & 63;
  const int64_t wg = (int64_t)blockIdx.x * kW + (threadIdx.x >> 6);
  const float count = (float)a.K;
  const int64_t j1 = min(a.n_v, (wg + 1) * a.rpw);
  for (int64_t j = wg * a.rpw; j < j1; ++j) {
    const typename G::Node nd = gr.node(j);
    // (s3 and s4 are summed again over every node into a bias gradient that is zero in exact arithmetic)
    const double s3 = node_sum<double, G>(nd.depot, nd.deg, [&](int t) {
      int64_t e, jj;
      gr.out(nd, t, a.nbr, e, jj);
      return (double)a.GUE[e * kD + lane];
    });
    const int p0 = a.ptr[j], n_in = a.ptr[j + 1] - p0;  // an in-degree of 0: both sums stay 0
    // where the sources' out-degrees differ each term of gx2 is divided by its own, otherwise the sum by the one there is
    const Incoming in = node_sum<Incoming, G>(nd.depot, n_in, [&](int t) {
      const int64_t e = a.src[p0 + t];
      int64_t i;
      float deg;
      gr.source(nd, e, i, deg);
      const float v = sigm(a.W0[e * kD + lane]) * a.GUV[i * kD + lane];
      return Incoming{(double)a.GUE[e * kD + lane], G::kDepot ? v / deg : v};
    });
    const float s2 = in.g2;
    const double s4 = in.g4;
    a.G2[j * kD + lane] = G::kDepot ? s2 : s2 / count;
    a.G3[j * kD + lane] = (float)s3;
    a.G4[j * kD + lane] = (float)s4;
  }
}

// ---- the row passes over both sides at once (lane = four channels of every fourth row) -----------------------------------------
struct Side {
  const float* pre;    // [rows][64]
  const float* in;     // apply: x0 / w0; backward: the gradient of the layer's output
  float* out;          // apply: x / w; bwd_gu: gu
  const float* stat;   // mu [64], r [64]
  const float* gamma;
  const float* beta;
  const float* means;  // bwd_gu: mean gy [64], mean gy u^ [64], then what each leaves as a float [64], [64]
  float* part;         // [P][3][64]
  int64_t rows;
  int rpw, P;
};
struct RowArgs {
  const int* bad;
  Side s[2];
};
// (count, mean, M2) are combined in float64: the card's fp32 reference accumulates its batch statistics in float64 too, and
// over a few dozen rows a mean that is an ulp off shows in every gradient behind it
struct Stat {
  double n, mean, m2;
};
__device__ inline Stat merge(const Stat a, const Stat b) {  // Chan, Golub, LeVeque
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  const double n = a.n + b.n, d = b.mean - a.mean;
  return Stat{n, a.mean + d * (b.n / n), (a.m2 + b.m2) + (d * d) * (a.n * b.n / n)};
}
// the wave's rows [r0, r1) of the block's side; `blk`: the workgroup's index on its side
__device__ inline const Side& side_of(const RowArgs& a, int& blk) {
  const int sd = (int)blockIdx.x < a.s[0].P ? 0 : 1;
  blk = blockIdx.x - (sd ? a.s[0].P : 0);
  return a.s[sd];
}
__device__ inline f32x4 load4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

__global__ void __launch_bounds__(kT) k_row_stats(const RowArgs a) {
  __shared__ float sn[kW][4][16];
  __shared__ double smean[kW][4][kD];
  __shared__ double sm2[kW][4][kD];
  if (*a.bad) return;
  int blk;
  const Side& s = side_of(a, blk);
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4, w = threadIdx.x >> 6;
  const int64_t r0 = ((int64_t)blk * kW + w) * s.rpw, r1 = min(s.rows, r0 + s.rpw);
  double sum[4] = {0.0, 0.0, 0.0, 0.0}, m2[4] = {0.0, 0.0, 0.0, 0.0}, mean[4] = {0.0, 0.0, 0.0, 0.0};
  int cnt = 0;
  for (int64_t r = r0 + g; r < r1; r += 4) {
    const f32x4 v = load4(s.pre + r * kD + 4 * c);
#pragma unroll
    for (int q = 0; q < 4; ++q) sum[q] += (double)v[q];
    ++cnt;
  }
  if (cnt) {
#pragma unroll
    for (int q = 0; q < 4; ++q) mean[q] = sum[q] / (double)cnt;
  }
  for (int64_t r = r0 + g; r < r1; r += 4) {
    const f32x4 v = load4(s.pre + r * kD + 4 * c);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double d = (double)v[q] - mean[q];
      m2[q] += d * d;
    }
  }
  sn[w][g][c] = (float)cnt;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    smean[w][g][4 * c + q] = mean[q];
    sm2[w][g][4 * c + q] = m2[q];
  }
  __syncthreads();
  if (threadIdx.x < kD) {
    const int ch = threadIdx.x;
    Stat t{0.0, 0.0, 0.0};
    for (int ww = 0; ww < kW; ++ww)
      for (int gg = 0; gg < 4; ++gg) t = merge(t, Stat{(double)sn[ww][gg][ch >> 2], smean[ww][gg][ch], sm2[ww][gg][ch]});
    float* part = s.part + (int64_t)blk * 3 * kD;
    part[ch] = (float)t.n;
    part[kD + ch] = (float)t.mean;
    part[2 * kD + ch] = (float)t.m2;
  }
}

struct FinalArgs {
  const int* bad;
  const float* part[2];
  int P[2];
  float eps;
  float* stat;   // forward: this layer's [6][64]
  float* means;  // backward: [2][4][64]
  float *gbn_w, *gbn_b;  // backward: this layer's [2][64] each
  float rows[2];
};
// one workgroup of 1024 threads per side: sixteen runs of consecutive partials, then the sixteen in order
__global__ void __launch_bounds__(1024) k_stats_finalize(const FinalArgs a) {
  __shared__ double sh[16][3][kD];
  if (*a.bad) return;
  const int sd = blockIdx.x, q = threadIdx.x >> 6, ch = threadIdx.x & 63;
  const int P = a.P[sd], per = (P + 15) / 16;
  const float* part = a.part[sd];
  Stat t{0.0, 0.0, 0.0};
  for (int p = q * per; p < min(P, (q + 1) * per); ++p) {
    const float* row = part + (int64_t)p * 3 * kD;
    t = merge(t, Stat{(double)row[ch], (double)row[kD + ch], (double)row[2 * kD + ch]});
  }
  sh[q][0][ch] = t.n;
  sh[q][1][ch] = t.mean;
  sh[q][2][ch] = t.m2;
  __syncthreads();
  if (threadIdx.x < kD) {
    Stat u{0.0, 0.0, 0.0};
    for (int qq = 0; qq < 16; ++qq) u = merge(u, Stat{sh[qq][0][ch], sh[qq][1][ch], sh[qq][2][ch]});
    const double var = u.m2 / u.n;
    float* st = a.stat + sd * 3 * kD;
    st[ch] = (float)u.mean;
    st[kD + ch] = (float)(1.0 / sqrt(var + (double)a.eps));
    st[2 * kD + ch] = (float)var;
  }
}

__global__ void __launch_bounds__(kT) k_apply(const RowArgs a) {
  if (*a.bad) return;
  int blk;
  const Side& s = side_of(a, blk);
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4, w = threadIdx.x >> 6;
  const int64_t r0 = ((int64_t)blk * kW + w) * s.rpw, r1 = min(s.rows, r0 + s.rpw);
  const f32x4 mu = load4(s.stat + 4 * c), rs = load4(s.stat + kD + 4 * c), ga = load4(s.gamma + 4 * c), be = load4(s.beta + 4 * c);
  for (int64_t r = r0 + g; r < r1; r += 4) {
    const f32x4 u = load4(s.pre + r * kD + 4 * c), x0 = load4(s.in + r * kD + 4 * c);
    f32x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = x0[q] + silu(((u[q] - mu[q]) * rs[q]) * ga[q] + be[q]);
    *reinterpret_cast<f32x4*>(s.out + r * kD + 4 * c) = o;
  }
}

// gy = g silu'(y) and u^ of one element
__device__ inline void gy_of(float u, float gin, float mu, float rs, float ga, float be, float& gy, float& uh) {
  uh = (u - mu) * rs;
  const float y = uh * ga + be, sg = sigm(y);
  gy = gin * (sg * (1.0f + y * (1.0f - sg)));
}

__global__ void __launch_bounds__(kT) k_bwd_reduce(const RowArgs a) {
  __shared__ float s1[kW][4][kD];
  __shared__ float s2[kW][4][kD];
  if (*a.bad) return;
  int blk;
  const Side& s = side_of(a, blk);
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4, w = threadIdx.x >> 6;
  const int64_t r0 = ((int64_t)blk * kW + w) * s.rpw, r1 = min(s.rows, r0 + s.rpw);
  const f32x4 mu = load4(s.stat + 4 * c), rs = load4(s.stat + kD + 4 * c), ga = load4(s.gamma + 4 * c), be = load4(s.beta + 4 * c);
  f32x4 t1{0.0f, 0.0f, 0.0f, 0.0f}, t2{0.0f, 0.0f, 0.0f, 0.0f};
  for (int64_t r = r0 + g; r < r1; r += 4) {
    const f32x4 u = load4(s.pre + r * kD + 4 * c), gin = load4(s.in + r * kD + 4 * c);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float gy, uh;
      gy_of(u[q], gin[q], mu[q], rs[q], ga[q], be[q], gy, uh);
      t1[q] += gy;
      t2[q] += gy * uh;
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    s1[w][g][4 * c + q] = t1[q];
    s2[w][g][4 * c + q] = t2[q];
  }
  __syncthreads();
  if (threadIdx.x < kD) {
    const int ch = threadIdx.x;
    float u1 = 0.0f, u2 = 0.0f;
    for (int ww = 0; ww < kW; ++ww)
      for (int gg = 0; gg < 4; ++gg) {
        u1 += s1[ww][gg][ch];
        u2 += s2[ww][gg][ch];
      }
    float* part = s.part + (int64_t)blk * 3 * kD;
    part[ch] = u1;
    part[kD + ch] = u2;
  }
}

__global__ void __launch_bounds__(1024) k_bwd_finalize(const FinalArgs a) {
  __shared__ double sh[16][2][kD];
  if (*a.bad) return;
  const int sd = blockIdx.x, q = threadIdx.x >> 6, ch = threadIdx.x & 63;
  const int P = a.P[sd], per = (P + 15) / 16;
  const float* part = a.part[sd];
  double u1 = 0.0, u2 = 0.0;
  for (int p = q * per; p < min(P, (q + 1) * per); ++p) {
    u1 += (double)part[(int64_t)p * 3 * kD + ch];
    u2 += (double)part[(int64_t)p * 3 * kD + kD + ch];
  }
  sh[q][0][ch] = u1;
  sh[q][1][ch] = u2;
  __syncthreads();
  if (threadIdx.x < kD) {
    double v1 = 0.0, v2 = 0.0;
    for (int qq = 0; qq < 16; ++qq) {
      v1 += sh[qq][0][ch];
      v2 += sh[qq][1][ch];
    }
    a.gbn_b[sd * kD + ch] = (float)v1;
    a.gbn_w[sd * kD + ch] = (float)v2;
    // the means as a float and what it leaves: a rounded mean is off by the same amount in every row, and the sums over
    // all rows that follow (the linears' bias gradients, zero in exact arithmetic) would collect it rows times
    const double m1 = v1 / (double)a.rows[sd], m2 = v2 / (double)a.rows[sd];
    float* mean = a.means + sd * 4 * kD;
    mean[ch] = (float)m1;
    mean[kD + ch] = (float)m2;
    mean[2 * kD + ch] = (float)(m1 - (double)(float)m1);
    mean[3 * kD + ch] = (float)(m2 - (double)(float)m2);
  }
}

__global__ void __launch_bounds__(kT) k_bwd_gu(const RowArgs a) {
  if (*a.bad) return;
  int blk;
  const Side& s = side_of(a, blk);
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4, w = threadIdx.x >> 6;
  const int64_t r0 = ((int64_t)blk * kW + w) * s.rpw, r1 = min(s.rows, r0 + s.rpw);
  const f32x4 mu = load4(s.stat + 4 * c), rs = load4(s.stat + kD + 4 * c), ga = load4(s.gamma + 4 * c), be = load4(s.beta + 4 * c);
  const f32x4 m1 = load4(s.means + 4 * c), m2 = load4(s.means + kD + 4 * c);
  const f32x4 m1l = load4(s.means + 2 * kD + 4 * c), m2l = load4(s.means + 3 * kD + 4 * c);
  for (int64_t r = r0 + g; r < r1; r += 4) {
    const f32x4 u = load4(s.pre + r * kD + 4 * c), gin = load4(s.in + r * kD + 4 * c);
    f32x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float gy, uh;
      gy_of(u[q], gin[q], mu[q], rs[q], ga[q], be[q], gy, uh);
      o[q] = (ga[q] * rs[q]) * ((((gy - m1[q]) - m1l[q]) - uh * m2[q]) - uh * m2l[q]);
    }
    *reinterpret_cast<f32x4*>(s.out + r * kD + 4 * c) = o;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
template <class G>
int64_t workspace_bytes(int B, int N, int K, int L) {
  if (B < 1 || N < G::kMinN || N > 1024 || K < 1 || K > 64 || K > N - G::kMinN + 1 || L < 1 || L > (1 << 20)) return 0;
  const int64_t n_e = B * G(N, K).rows();
  if (n_e > (1 << 24)) return 0;
  return layout((int64_t)B * N, n_e, L).total * 4;
}

template <class G, class A>
int require_common(const A& a) {
  RL4CO_REQUIRE(a.D == kD);
  RL4CO_REQUIRE(a.B >= 1);
  RL4CO_REQUIRE(a.N >= G::kMinN && a.N <= 1024);
  RL4CO_REQUIRE(a.K >= 1 && a.K <= 64 && a.K <= a.N - G::kMinN + 1);  // (the depot has no kNN row)
  RL4CO_REQUIRE(a.L >= 1 && a.L <= (1 << 20));
  RL4CO_REQUIRE(a.B * G(a.N, a.K).rows() <= (1 << 24));  // row counts are exact in fp32, row indices fit an int32
  RL4CO_REQUIRE(a.reserved0 == 0 && a.reserved1 == 0);
  RL4CO_REQUIRE(a.eps > 0.0f);
  RL4CO_REQUIRE(a.neighbors != nullptr && a.csr_ptr != nullptr && a.csr_src != nullptr);
  RL4CO_REQUIRE(a.x_in != nullptr && a.w_in != nullptr);
  RL4CO_REQUIRE(a.lin_w != nullptr && a.lin_b != nullptr && a.bn_w != nullptr && a.bn_b != nullptr);
  RL4CO_REQUIRE(a.workspace != nullptr && a.stats != nullptr && a.err != nullptr);
  RL4CO_REQUIRE(a.workspace_bytes >= workspace_bytes<G>(a.B, a.N, a.K, a.L));
  const uintptr_t all = reinterpret_cast<uintptr_t>(a.x_in) | reinterpret_cast<uintptr_t>(a.w_in) |
                        reinterpret_cast<uintptr_t>(a.lin_w) | reinterpret_cast<uintptr_t>(a.bn_w) |
                        reinterpret_cast<uintptr_t>(a.bn_b) | reinterpret_cast<uintptr_t>(a.workspace) |
                        reinterpret_cast<uintptr_t>(a.stats);
  RL4CO_REQUIRE((all & 15) == 0);  // 16-byte fragments
  return RL4CO_OK;
}

// the flag is cleared and the lists are checked before any other launch of the call
template <class G, class A>
int launch_check(const A& a, hipStream_t s) {
  RL4CO_HIP_TRY(hipMemsetAsync(a.workspace, 0, kHead * 4, s));
  const G gr(a.N, a.K);
  CheckArgs c{a.neighbors, a.csr_ptr, a.csr_src, (int64_t)a.B * a.N, a.B * gr.rows(), a.B * gr.lists(), a.N, a.K,
              reinterpret_cast<int*>(a.workspace), a.err};
  const int grid = (int)std::min<int64_t>((c.n_e + kT - 1) / kT, kMaxGroups);
  hipLaunchKernelGGL(k_check<G>, dim3(grid), dim3(kT), 0, s, c);
  RL4CO_HIP_TRY(hipGetLastError());
  return RL4CO_OK;
}

struct Shape {
  Layout y;
  int64_t n_v, n_e;
  int rpw_v, rpw_e;  // rows per wave (16 tiles_per_wave)
};
template <class G, class A>
Shape shape_of(const A& a) {
  Shape h;
  h.n_v = (int64_t)a.B * a.N;
  h.n_e = a.B * G(a.N, a.K).rows();
  h.y = layout(h.n_v, h.n_e, a.L);
  h.rpw_v = 16 * tiles_per_wave(h.n_v, h.y.Pv);
  h.rpw_e = 16 * tiles_per_wave(h.n_e, h.y.Pe);
  return h;
}

template <class G, class A>
int forward(const A* args, void* stream) {
  RL4CO_REQUIRE(args != nullptr);
  const A& a = *args;
  if (const int rc = require_common<G>(a)) return rc;
  RL4CO_REQUIRE(a.x_out != nullptr && a.w_out != nullptr);
  RL4CO_REQUIRE(((reinterpret_cast<uintptr_t>(a.x_out) | reinterpret_cast<uintptr_t>(a.w_out)) & 15) == 0);
  hipStream_t s = rl4co::as_stream(stream);
  if (const int rc = launch_check<G>(a, s)) return rc;
  const Shape h = shape_of<G>(a);
  const Layout& y = h.y;
  float* ws = a.workspace;
  const int* bad = reinterpret_cast<const int*>(ws);
  float* T = ws + y.t;
  for (int l = 0; l < a.L; ++l) {
    const float* x0 = l == 0 ? a.x_in : ws + y.xs + (int64_t)(l - 1) * y.nv;
    const float* w0 = l == 0 ? a.w_in : ws + y.ws + (int64_t)(l - 1) * y.ne;
    float* x = l == a.L - 1 ? a.x_out : ws + y.xs + (int64_t)l * y.nv;
    float* w = l == a.L - 1 ? a.w_out : ws + y.ws + (int64_t)l * y.ne;
    float* pv = ws + y.pv + (int64_t)l * y.nv;
    float* pe = ws + y.pe + (int64_t)l * y.ne;
    float* x2 = ws + y.x2 + (int64_t)l * y.nv;
    const float* LW = a.lin_w + (int64_t)l * 5 * kD * kD;
    const float* LB = a.lin_b + (int64_t)l * 5 * kD;
    float* stat = a.stats + (int64_t)l * 6 * kD;

    LinFwdArgs nf{bad, x0, LW, LB, {T, x2, T + 2 * y.nv, T + 3 * y.nv}, h.n_v, h.rpw_v / 16, nullptr, nullptr, a.neighbors, a.N, a.K};
    hipLaunchKernelGGL((k_lin_fwd<false, G>), dim3(y.Pv, 4), dim3(kT), 0, s, nf);
    NodeArgs na{};
    na.bad = bad, na.nbr = a.neighbors, na.W0 = w0, na.X1 = T, na.X2 = x2, na.PV = pv;
    na.n_v = h.n_v, na.rpw = h.rpw_v, na.N = a.N, na.K = a.K;
    hipLaunchKernelGGL(k_vert_pre<G>, dim3(y.Pv), dim3(kT), 0, s, na);
    LinFwdArgs ef{bad, w0, LW + 4 * kD * kD, LB + 4 * kD, {pe, nullptr, nullptr, nullptr}, h.n_e, h.rpw_e / 16,
                  T + 2 * y.nv, T + 3 * y.nv, a.neighbors, a.N, a.K};
    hipLaunchKernelGGL((k_lin_fwd<true, G>), dim3(y.Pe), dim3(kT), 0, s, ef);

    float* part_v = ws + y.part;
    float* part_e = part_v + (int64_t)192 * y.Pv;
    RowArgs ra{};
    ra.bad = bad;
    ra.s[0] = Side{pv, x0, x, stat, a.bn_w + (int64_t)l * 2 * kD, a.bn_b + (int64_t)l * 2 * kD, nullptr, part_v, h.n_v, h.rpw_v, y.Pv};
    ra.s[1] = Side{pe, w0, w, stat + 3 * kD, a.bn_w + (int64_t)l * 2 * kD + kD, a.bn_b + (int64_t)l * 2 * kD + kD, nullptr, part_e,
                   h.n_e, h.rpw_e, y.Pe};
    hipLaunchKernelGGL(k_row_stats, dim3(y.Pv + y.Pe), dim3(kT), 0, s, ra);
    FinalArgs fa{};
    fa.bad = bad, fa.part[0] = part_v, fa.part[1] = part_e, fa.P[0] = y.Pv, fa.P[1] = y.Pe, fa.eps = a.eps, fa.stat = stat;
    hipLaunchKernelGGL(k_stats_finalize, dim3(2), dim3(1024), 0, s, fa);
    hipLaunchKernelGGL(k_apply, dim3(y.Pv + y.Pe), dim3(kT), 0, s, ra);
    RL4CO_HIP_TRY(hipGetLastError());
  }
  return RL4CO_OK;
}

template <class G, class A>
int backward(const A* args, void* stream) {
  RL4CO_REQUIRE(args != nullptr);
  const A& a = *args;
  if (const int rc = require_common<G>(a)) return rc;
  RL4CO_REQUIRE(a.grad_x_out != nullptr && a.grad_w_out != nullptr && a.grad_x_in != nullptr && a.grad_w_in != nullptr);
  RL4CO_REQUIRE(a.grad_lin_w != nullptr && a.grad_lin_b != nullptr && a.grad_bn_w != nullptr && a.grad_bn_b != nullptr);
  const uintptr_t all = reinterpret_cast<uintptr_t>(a.grad_x_out) | reinterpret_cast<uintptr_t>(a.grad_w_out) |
                        reinterpret_cast<uintptr_t>(a.grad_x_in) | reinterpret_cast<uintptr_t>(a.grad_w_in);
  RL4CO_REQUIRE((all & 15) == 0);
  hipStream_t s = rl4co::as_stream(stream);
  if (const int rc = launch_check<G>(a, s)) return rc;
  const Shape h = shape_of<G>(a);
  const Layout& y = h.y;
  float* ws = a.workspace;
  const int* bad = reinterpret_cast<const int*>(ws);
  float* T = ws + y.t;
  float* GX = ws + y.gx;
  float* GW = ws + y.gw;
  float* GUE = ws + y.gue;
  float* means = ws + y.means;
  float* part_v = ws + y.part;
  float* part_e = part_v + (int64_t)192 * y.Pv;
  float* dwp = ws + y.dw;
  for (int l = a.L - 1; l >= 0; --l) {
    const float* x0 = l == 0 ? a.x_in : ws + y.xs + (int64_t)(l - 1) * y.nv;
    const float* w0 = l == 0 ? a.w_in : ws + y.ws + (int64_t)(l - 1) * y.ne;
    const float* pv = ws + y.pv + (int64_t)l * y.nv;
    const float* pe = ws + y.pe + (int64_t)l * y.ne;
    const float* x2 = ws + y.x2 + (int64_t)l * y.nv;
    const float* LW = a.lin_w + (int64_t)l * 5 * kD * kD;
    const float* stat = a.stats + (int64_t)l * 6 * kD;
    const float* gx = l == a.L - 1 ? a.grad_x_out : GX;  // the gradients of this layer's outputs
    const float* gw = l == a.L - 1 ? a.grad_w_out : GW;
    float* gx0 = l == 0 ? a.grad_x_in : GX;
    float* gw0 = l == 0 ? a.grad_w_in : GW;

    RowArgs ra{};
    ra.bad = bad;
    ra.s[0] = Side{pv, gx, T, stat, a.bn_w + (int64_t)l * 2 * kD, a.bn_b + (int64_t)l * 2 * kD, means, part_v, h.n_v, h.rpw_v, y.Pv};
    ra.s[1] = Side{pe, gw, GUE, stat + 3 * kD, a.bn_w + (int64_t)l * 2 * kD + kD, a.bn_b + (int64_t)l * 2 * kD + kD, means + 4 * kD,
                   part_e, h.n_e, h.rpw_e, y.Pe};
    hipLaunchKernelGGL(k_bwd_reduce, dim3(y.Pv + y.Pe), dim3(kT), 0, s, ra);
    FinalArgs fa{};
    fa.bad = bad, fa.part[0] = part_v, fa.part[1] = part_e, fa.P[0] = y.Pv, fa.P[1] = y.Pe, fa.means = means;
    fa.gbn_w = a.grad_bn_w + (int64_t)l * 2 * kD, fa.gbn_b = a.grad_bn_b + (int64_t)l * 2 * kD;
    fa.rows[0] = (float)h.n_v, fa.rows[1] = (float)h.n_e;
    hipLaunchKernelGGL(k_bwd_finalize, dim3(2), dim3(1024), 0, s, fa);
    hipLaunchKernelGGL(k_bwd_gu, dim3(y.Pv + y.Pe), dim3(kT), 0, s, ra);

    LinBwdArgs eb{bad, GUE, w0, LW + 4 * kD * kD, gw, gw0, dwp + (int64_t)4 * y.Pv * kPartDw, h.n_e, h.rpw_e / 16,
                  T, x2, a.neighbors, a.N, a.K};
    hipLaunchKernelGGL((k_lin_bwd<true, G>), dim3(y.Pe), dim3(kT), 0, s, eb);
    NodeArgs na{};
    na.bad = bad, na.nbr = a.neighbors, na.ptr = a.csr_ptr, na.src = a.csr_src, na.W0 = w0, na.GUE = GUE, na.GUV = T;
    na.G2 = T + y.nv, na.G3 = T + 2 * y.nv, na.G4 = T + 3 * y.nv;
    na.n_v = h.n_v, na.rpw = h.rpw_v, na.N = a.N, na.K = a.K;
    hipLaunchKernelGGL(k_node_bwd<G>, dim3(y.Pv), dim3(kT), 0, s, na);
    for (int m = 0; m < 4; ++m) {
      LinBwdArgs nb{bad, T + (int64_t)m * y.nv, x0, LW + m * kD * kD, m == 0 ? gx : gx0, gx0, dwp + (int64_t)m * y.Pv * kPartDw,
                    h.n_v, h.rpw_v / 16, nullptr, nullptr, a.neighbors, a.N, a.K};
      hipLaunchKernelGGL((k_lin_bwd<false, G>), dim3(y.Pv), dim3(kT), 0, s, nb);
    }
    DwFinalArgs df{bad, dwp, y.Pv, y.Pe, a.grad_lin_w + (int64_t)l * 5 * kD * kD, a.grad_lin_b + (int64_t)l * 5 * kD};
    hipLaunchKernelGGL(k_dw_finalize, dim3((kPartDw + kT - 1) / kT, 5), dim3(kT), 0, s, df);
    RL4CO_HIP_TRY(hipGetLastError());
  }
  return RL4CO_OK;
}

}  // namespace

extern "C" int64_t rl4co_nargnn_train_workspace_bytes(int B, int N, int K, int L) { return workspace_bytes<Regular>(B, N, K, L); }
extern "C" int rl4co_nargnn_train_forward(const rl4co_nargnn_train_args* args, void* stream) {
  return forward<Regular>(args, stream);
}
extern "C" int rl4co_nargnn_train_backward(const rl4co_nargnn_train_args* args, void* stream) {
  return backward<Regular>(args, stream);
}

extern "C" int64_t rl4co_nargnn_depot_train_workspace_bytes(int B, int N, int K, int L) {
  return workspace_bytes<Depot>(B, N, K, L);
}
extern "C" int rl4co_nargnn_depot_train_forward(const rl4co_nargnn_depot_train_args* args, void* stream) {
  return forward<Depot>(args, stream);
}
extern "C" int rl4co_nargnn_depot_train_backward(const rl4co_nargnn_depot_train_args* args, void* stream) {
  return backward<Depot>(args, stream);
}
