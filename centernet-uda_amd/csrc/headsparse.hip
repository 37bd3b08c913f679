// The backward of a detection head (conv kh x kw + act + conv 1x1, dla.py:474-483) for a gradient that is zero outside a
// handful of cells: the `wh` / `reg` heads under the gather + masked-L1 loss (loss.hip, regl1_bwd_kernel) receive a
// [B, Co, H, W] map with at most M non-zero pixels per image.  The dense chain (conv1x1_dgrad_act_kernel over the whole hidden
// map, two full-size 3x3 GEMMs) multiplies by exact zeros everywhere else.  Here the R = B * M candidate rows are gathered
// into compact [channels][R] matrices -- NCHW "images" of batch 1, height 1, width R -- and the SAME sums are taken by the
// 1x1 convolution entry points over them:
//   grad_w2, grad_b2 = cnuda_conv2d_backward_weight(hrow [Ch][R], gyrow [Co][R])
//   grad_w1, grad_b1 = cnuda_conv2d_backward_weight(xp [C T][R], gh [Ch][R])      ([Ch, C T, 1, 1] IS [Ch, C, kh, kw]: xp's channel is c T + tap)
//   t [C T][R]       = cnuda_conv2d_backward_data(gh, w1 as [Ch, C T, 1, 1])
//   grad_x[b][c][y + ky - ph][x + kx - pw] += t[c T + ky kw + kx][r]             (plain read-add-write in a fixed order, no atomics)
// Inactive and padding rows are zeros in every matrix: the launches are the same every step, whatever the batch holds.
#include <algorithm>

#include "igemm_host.h"

namespace cnuda {
namespace {

constexpr int kRows = 64;        // rows of a workgroup: one wavefront wide, so every store is a coalesced 256-byte line
constexpr int kChunk = 32;       // compact channels per workgroup, dealt round-robin to its four wavefronts
constexpr int kThreads = 256;
constexpr int kMaxCo = 8, kMaxM = 4096;      // (M: the duplicate scan is O(M) per row)

struct HeadGeom {
    int B, M, C, H, W, Ch, Co, kh, kw, ph, pw, T, R;
    long long HW;
};

// Row r = (b, m) is ACTIVE when mask[b][m] is set, ind[b][m] lies in [0, HW) (loss.hip's ind_ok: a row outside never touches
// memory) and no m' < m of the same image is masked with the same ind -- regl1_bwd_kernel ADDED the duplicates into one cell,
// which must be read once.  -> the pixel of the row, -1 for an inactive or padding row.  *crowded: another masked row of the
// image lies within kh - 1 rows and kw - 1 columns, i.e. the two patches share cells of grad_x (head_scatter_kernel).
// `flags`: 2 * kRows ints of LDS; the four wavefronts of the workgroup split the scan over m'.
__device__ __forceinline__ int head_row_pixel(const HeadGeom& g, const long long* __restrict__ ind,
                                              const unsigned char* __restrict__ mask, int r, int lane, int sub, int* flags,
                                              bool* crowded) {
    int *dup = flags, *near = flags + kRows;
    if (sub == 0) dup[lane] = near[lane] = 0;
    __syncthreads();
    const bool real = r < g.B * g.M;
    const int b = real ? r / g.M : 0, m = real ? r - b * g.M : 0;
    const long long id = real ? ind[r] : -1;
    const bool ok = real && mask[r] != 0 && id >= 0 && id < g.HW;
    if (ok) {
        const int y = (int)(id / g.W), x = (int)(id - (long long)y * g.W);
        bool seen = false, close = false;
        for (int k = sub; k < g.M; k += kThreads / kRows) {
            const long long other = ind[b * g.M + k];
            if (k == m || mask[b * g.M + k] == 0 || other < 0 || other >= g.HW) continue;
            seen |= k < m && other == id;
            const int oy = (int)(other / g.W), ox = (int)(other - (long long)oy * g.W);
            close |= abs(oy - y) <= 2 * g.ph && abs(ox - x) <= 2 * g.pw;
        }
        if (seen) dup[lane] = 1;
        if (close) near[lane] = 1;
    }
    __syncthreads();
    *crowded = near[lane] != 0;
    return ok && dup[lane] == 0 ? (int)id : -1;
}

// grid (R / kRows, (Co + Ch + C T) / kChunk): compact channel j is a row of gyrow (j < Co), of hrow AND gh (the next Ch), or
// of xp (the rest).  Scattered 4-byte reads, coalesced writes along r.
__global__ __launch_bounds__(kThreads) void head_rows_kernel(HeadGeom g, const float* __restrict__ gy, const long long* __restrict__ ind,
                                                             const unsigned char* __restrict__ mask, const float* __restrict__ x,
                                                             const float* __restrict__ hid, const float* __restrict__ w2, float slope,
                                                             float* __restrict__ gyrow, float* __restrict__ hrow, float* __restrict__ gh,
                                                             float* __restrict__ xp, int* __restrict__ rowpix,
                                                             int* __restrict__ rowcrowd) {
    __shared__ int flags[2 * kRows];
    const int lane = threadIdx.x & (kRows - 1), sub = threadIdx.x / kRows, r = blockIdx.x * kRows + lane;
    bool crowded;
    const int pix = head_row_pixel(g, ind, mask, r, lane, sub, flags, &crowded);
    if (r >= g.R) return;
    if (blockIdx.y == 0 && sub == 0) { rowpix[r] = pix; rowcrowd[r] = crowded ? 1 : 0; }
    const int b = pix >= 0 ? r / g.M : 0, py = pix >= 0 ? pix / g.W : 0, px = pix >= 0 ? pix - py * g.W : 0;
    float go[kMaxCo];
#pragma unroll
    for (int c = 0; c < kMaxCo; ++c) go[c] = (pix >= 0 && c < g.Co) ? gy[((size_t)b * g.Co + c) * g.HW + pix] : 0.0f;
    const int J = g.Co + g.Ch + g.C * g.T;
    for (int j = blockIdx.y * kChunk + sub; j < min((int)(blockIdx.y + 1) * kChunk, J); j += kThreads / kRows) {
        if (j < g.Co) {
            float v = 0.0f;
#pragma unroll
            for (int c = 0; c < kMaxCo; ++c) if (c == j) v = go[c];
            gyrow[(size_t)j * g.R + r] = v;
        } else if (j < g.Co + g.Ch) {
            const int ch = j - g.Co;
            float h = 0.0f, o = 0.0f;
            if (pix >= 0) {
                h = hid[((size_t)b * g.Ch + ch) * g.HW + pix];
                // (the expression and the channel order of conv1x1_dgrad_act_kernel, spatial.hip)
#pragma unroll
                for (int c = 0; c < kMaxCo; ++c) if (c < g.Co) o += w2[(size_t)c * g.Ch + ch] * go[c];
                o = h > 0.0f ? o : o * slope;
            }
            hrow[(size_t)ch * g.R + r] = h;
            gh[(size_t)ch * g.R + r] = o;
        } else {
            const int q = j - g.Co - g.Ch, c = q / g.T, tap = q - c * g.T, ky = tap / g.kw, kx = tap - ky * g.kw;
            const int yy = py + ky - g.ph, xx = px + kx - g.pw;
            const bool in = pix >= 0 && yy >= 0 && yy < g.H && xx >= 0 && xx < g.W;
            xp[(size_t)q * g.R + r] = in ? x[((size_t)b * g.C + c) * g.HW + (size_t)yy * g.W + xx] : 0.0f;
        }
    }
}

// grad_x[b][c][y + ky - ph][x + kx - pw] += t[c T + tap][r] for the active rows, where the target lies inside the image, with
// plain read-add-write in an order that does not depend on scheduling (the step's gradients stay bit-reproducible):
//   blockIdx.x <  row_blocks: the rows with no other row near them (rowcrowd == 0) own their cells; 64 rows x kChunk of the
//                             C T patch channels per workgroup (blockIdx.y), all in parallel;
//   blockIdx.x >= row_blocks: image b = blockIdx.x - row_blocks, kScatterC whole channels (blockIdx.y; every tap of a channel
//                             in ONE workgroup): the crowded rows of the image one after the other in row order, a barrier
//                             between two of them.  Their cells are disjoint from every lone row's.
constexpr int kScatterC = 4;
__global__ __launch_bounds__(kThreads) void head_scatter_kernel(HeadGeom g, const float* __restrict__ t, const int* __restrict__ rowpix,
                                                                const int* __restrict__ rowcrowd, float* __restrict__ gx, int row_blocks) {
    auto add = [&](int r, int b, int pix, int q) {
        const int py = pix / g.W, px = pix - py * g.W;
        const int c = q / g.T, tap = q - c * g.T, ky = tap / g.kw, kx = tap - ky * g.kw;
        const int yy = py + ky - g.ph, xx = px + kx - g.pw;
        if (yy >= 0 && yy < g.H && xx >= 0 && xx < g.W) gx[((size_t)b * g.C + c) * g.HW + (size_t)yy * g.W + xx] += t[(size_t)q * g.R + r];
    };
    const int Q = g.C * g.T;
    if ((int)blockIdx.x < row_blocks) {
        const int lane = threadIdx.x & (kRows - 1), sub = threadIdx.x / kRows, r = blockIdx.x * kRows + lane;
        if (r >= g.B * g.M) return;
        const int pix = rowpix[r];
        if (pix < 0 || rowcrowd[r] != 0) return;
        for (int q = blockIdx.y * kChunk + sub; q < min((int)(blockIdx.y + 1) * kChunk, Q); q += kThreads / kRows) add(r, r / g.M, pix, q);
        return;
    }
    const int b = blockIdx.x - row_blocks, q0 = blockIdx.y * kScatterC * g.T, q1 = min(q0 + kScatterC * g.T, Q);
    if (q0 >= Q) return;
    for (int m = 0; m < g.M; ++m) {                     // (pix and the flag are uniform over the workgroup: so is the barrier)
        const int r = b * g.M + m, pix = rowpix[r];
        if (pix < 0 || rowcrowd[r] == 0) continue;
        for (int q = q0 + threadIdx.x; q < q1; q += kThreads) add(r, b, pix, q);
        __syncthreads();
    }
}

bool head_geom_ok(int B, int M, int C, int H, int W, int Ch, int Co, int kh, int kw, int sh, int sw, int ph, int pw) {
    return B > 0 && M > 0 && C > 0 && H > 0 && W > 0 && Ch > 0 && sh == 1 && sw == 1 && Co >= 1 && Co <= kMaxCo && kh == kw &&
           kh % 2 == 1 && kh <= 7 && ph == (kh - 1) / 2 && pw == ph && M <= kMaxM && (long long)B * M < (1 << 20) &&
           (long long)H * W < (1ll << 31) && (long long)C * kh * kw < (1 << 20);
}
HeadGeom head_geom(int B, int M, int C, int H, int W, int Ch, int Co, int kh, int kw) {
    return HeadGeom{B, M, C, H, W, Ch, Co, kh, kw, (kh - 1) / 2, (kw - 1) / 2, kh * kw, round_up(B * M, 4), (long long)H * W};
}
// the two 1x1 geometries over the compact matrices: (hrow -> gyrow) and (xp -> gh); their calls share one tail of the workspace
size_t head_gemm_bytes(const HeadGeom& g) {
    return std::max(cnuda_conv2d_workspace_bytes(1, g.Ch, 1, g.R, g.Co, 1, 1, 1, 1, 0, 0),
                    cnuda_conv2d_workspace_bytes(1, g.C * g.T, 1, g.R, g.Ch, 1, 1, 1, 1, 0, 0));
}
size_t head_rows_bytes(const HeadGeom& g) {
    return carve_bytes((size_t)g.Co * g.R, 4) + 2 * carve_bytes((size_t)g.Ch * g.R, 4) + 2 * carve_bytes((size_t)g.C * g.T * g.R, 4) +
           2 * carve_bytes(g.R, 4);
}

}  // namespace
}  // namespace cnuda

using namespace cnuda;

extern "C" int cnuda_head_backward_sparse_supported(int B, int M, int C, int H, int W, int Ch, int Co, int kh, int kw, int sh,
                                                    int sw, int ph, int pw) {
    return head_geom_ok(B, M, C, H, W, Ch, Co, kh, kw, sh, sw, ph, pw) ? 1 : 0;
}

extern "C" size_t cnuda_head_backward_sparse_workspace_bytes(int B, int M, int C, int H, int W, int Ch, int Co, int kh, int kw) {
    if (!head_geom_ok(B, M, C, H, W, Ch, Co, kh, kw, 1, 1, (kh - 1) / 2, (kw - 1) / 2)) {
        set_error("cnuda_head_backward_sparse_workspace_bytes: unsupported geometry (cnuda_head_backward_sparse_supported)");
        return 0;
    }
    const HeadGeom g = head_geom(B, M, C, H, W, Ch, Co, kh, kw);
    return head_rows_bytes(g) + head_gemm_bytes(g) + 512;
}

extern "C" int cnuda_head_backward_sparse(const float* grad_y, const long long* ind, const unsigned char* mask, const float* x,
                                          const float* hidden, const float* w1, const float* w2, float* grad_x, float* grad_w1,
                                          float* grad_b1, float* grad_w2, float* grad_b2, int B, int M, int C, int H, int W,
                                          int Ch, int Co, int kh, int kw, float slope, void* workspace, size_t workspace_bytes,
                                          cnuda_stream_t stream) {
    CNUDA_REQUIRE(grad_y && ind && mask && x && hidden && w1 && w2, "cnuda_head_backward_sparse: null pointer");
    CNUDA_REQUIRE(head_geom_ok(B, M, C, H, W, Ch, Co, kh, kw, 1, 1, (kh - 1) / 2, (kw - 1) / 2),
                  "cnuda_head_backward_sparse: unsupported geometry (cnuda_head_backward_sparse_supported)");
    CNUDA_REQUIRE((grad_w1 || !grad_b1) && (grad_w2 || !grad_b2), "cnuda_head_backward_sparse: a bias gradient comes with its weight gradient");
    const HeadGeom g = head_geom(B, M, C, H, W, Ch, Co, kh, kw);
    const size_t gemm_bytes = head_gemm_bytes(g);
    CNUDA_REQUIRE(workspace && workspace_bytes >= head_rows_bytes(g) + gemm_bytes + 512, "cnuda_head_backward_sparse: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    Carver cv(workspace, workspace_bytes);
    const int Q = C * g.T;
    float* gyrow = cv.take<float>((size_t)Co * g.R);
    float* hrow = cv.take<float>((size_t)Ch * g.R);
    float* gh = cv.take<float>((size_t)Ch * g.R);
    float* xp = cv.take<float>((size_t)Q * g.R);
    float* t = cv.take<float>((size_t)Q * g.R);
    int* rowpix = cv.take<int>(g.R);
    int* rowcrowd = cv.take<int>(g.R);
    void* gemm_ws = cv.take<char>(gemm_bytes);
    CNUDA_REQUIRE(cv.ok(), "cnuda_head_backward_sparse: workspace too small");

    const int row_blocks = ceil_div(g.R, kRows);
    CNUDA_LAUNCH(head_rows_kernel, dim3(row_blocks, ceil_div(Co + Ch + Q, kChunk)), dim3(kThreads), 0, st, g, grad_y, ind, mask, x,
                 hidden, w2, slope, gyrow, hrow, gh, xp, rowpix, rowcrowd);
    if (int rc = check_launch("cnuda_head_backward_sparse(rows)")) return rc;
    if (grad_w2)
        if (int rc = cnuda_conv2d_backward_weight(hrow, gyrow, grad_w2, grad_b2, 1, Ch, 1, g.R, Co, 1, 1, 1, 1, 0, 0, gemm_ws, gemm_bytes, stream))
            return rc;
    if (grad_w1)
        if (int rc = cnuda_conv2d_backward_weight(xp, gh, grad_w1, grad_b1, 1, Q, 1, g.R, Ch, 1, 1, 1, 1, 0, 0, gemm_ws, gemm_bytes, stream))
            return rc;
    if (grad_x) {
        if (int rc = cnuda_conv2d_backward_data(gh, w1, t, 1, Q, 1, g.R, Ch, 1, 1, 1, 1, 0, 0, gemm_ws, gemm_bytes, stream)) return rc;
        // (kChunk <= kScatterC * T may not hold for a 1x1 layer: the grid's y extent covers both partitions)
        const int lone_blocks = ceil_div((long long)B * M, kRows);
        CNUDA_LAUNCH(head_scatter_kernel, dim3(lone_blocks + B, std::max(ceil_div(Q, kChunk), ceil_div(C, kScatterC))), dim3(kThreads), 0, st, g,
                     t, rowpix, rowcrowd, grad_x, lone_blocks);
        if (int rc = check_launch("cnuda_head_backward_sparse(scatter)")) return rc;
    }
    return 0;
}
