// Deformable position-sensitive ROI pooling (DCNv2's second operator: libs/DCNv2/src/cuda/dcn_v2_psroi_pooling_cuda.cu,
// float instantiation), forward and backward, for gfx950.  fp32, NCHW.
//
//   forward      psroi_bins_kernel<false>     lane = bin (ph, pw) of one ROI, loop over a slice of output channels
//   grad_offset  psroi_bins_kernel<true>      same mapping: per (n, ctop, ph, pw) the two sums over the bin's samples
//                psroi_offset_reduce_kernel   one wave per offset element: channels of the class x bins of the part
//                                             cell, lane-strided sums in index order, then a fixed xor tree
//   grad_input   psroi_roi_lists_kernel       per image the ROIs that name it, in index order
//                psroi_grad_input_kernel      one wave owns a tile of rows of one (image, channel) plane in LDS and
//                                             GATHERS: ROIs in index order, bins in (ph, pw) order, every pixel of a
//                                             bin's footprint owned by one lane
// No floating-point atomics anywhere: every sum has one fixed order, so results are bit-stable from run to run.
//
// The three index expressions of the reference that land on either side of an integer depending on the precision --
// floor(float(ph) / P * part), floor(float(pw) * group / P) -- are evaluated once on the host in IEEE float, in that
// operation order, and travel to the kernels as two byte tables in the argument block (P <= 64).
#include <math.h>

#include <vector>

#include "common.h"

namespace cnuda {
namespace {

constexpr int kMaxPooled = 64;
constexpr int kMaxTileFloats = 16384;        // 64 KiB of LDS per plane tile: no opt-in needed

struct Psroi {
    const float* input;      // [B, C, H, W]
    const float* rois;       // [N, 5]
    const float* trans;      // [N, 2 * nc, part, part] or null (no_trans)
    int B, C, H, W, N, no_trans, OD, G, P, part, S, nc, cec;
    float scale, tstd;
    unsigned char part_of[kMaxPooled];       // floor(float(p) / P * part)
    unsigned char g_of[kMaxPooled];          // clamp(floor(float(p) * G / P), 0, G - 1)
};

struct RoiGeom {
    int b;
    float sw, sh, rw, rh, bw, bh, subw, subh;
};

__device__ __forceinline__ RoiGeom roi_geom(const Psroi& a, int n) {
    const float* r = a.rois + (size_t)n * 5;
    RoiGeom g;
    g.b = (int)r[0];
    // roundf: half away from zero, as C round()
    g.sw = roundf(r[1]) * a.scale - 0.5f;
    g.sh = roundf(r[2]) * a.scale - 0.5f;
    const float ew = (roundf(r[3]) + 1.0f) * a.scale - 0.5f;
    const float eh = (roundf(r[4]) + 1.0f) * a.scale - 0.5f;
    g.rw = fmaxf(ew - g.sw, 0.1f);
    g.rh = fmaxf(eh - g.sh, 0.1f);
    g.bw = g.rw / (float)a.P;
    g.bh = g.rh / (float)a.P;
    g.subw = g.bw / (float)a.S;
    g.subh = g.bh / (float)a.S;
    return g;
}

// first sample of bin (ph, pw) for class `cls` of ROI n
__device__ __forceinline__ void bin_start(const Psroi& a, const RoiGeom& g, int n, int cls, int ph, int pw, float& ws,
                                          float& hs) {
    float tx = 0.0f, ty = 0.0f;
    if (!a.no_trans) {
        const size_t cell = (size_t)a.part_of[ph] * a.part + a.part_of[pw];
        const size_t pp = (size_t)a.part * a.part;
        const float* t = a.trans + ((size_t)n * a.nc + cls) * 2 * pp;
        tx = t[cell] * a.tstd;
        ty = t[pp + cell] * a.tstd;
    }
    ws = (float)pw * g.bw + g.sw;
    ws += tx * g.rw;
    hs = (float)ph * g.bh + g.sh;
    hs += ty * g.rh;
}

__device__ __forceinline__ bool outside(float v, int size) { return v < -0.5f || v > (float)size - 0.5f; }
__device__ __forceinline__ float clamp_to(float v, int size) { return fminf(fmaxf(v, 0.0f), (float)size - 1.0f); }

// GRAD = false: out0 = pooled output, out1 = sample count.
// GRAD = true : out0 = [N, OD, P, P, 2] partial sums of the offset gradient (x, y) of every bin; go / cnt read.
// grid.x = N * ceil(P*P / 64), grid.y = slices of `cpw` output channels; one wave per block.  Neighbouring lanes are
// neighbouring pw of one bin row: for group_size 1 they gather neighbouring x of one channel plane.
template <bool GRAD>
__global__ __launch_bounds__(kWave) void psroi_bins_kernel(Psroi a, int cpw, const float* __restrict__ go,
                                                           const float* __restrict__ cnt, float* __restrict__ out0,
                                                           float* __restrict__ out1) {
    const int PP = a.P * a.P, chunks = (PP + kWave - 1) / kWave;
    const int n = blockIdx.x / chunks, bin = (blockIdx.x % chunks) * kWave + threadIdx.x;
    if (bin >= PP) return;
    const int ph = bin / a.P, pw = bin - ph * a.P;
    const RoiGeom g = roi_geom(a, n);
    const int gh = a.g_of[ph], gw = a.g_of[pw];
    const size_t hw = (size_t)a.H * a.W;
    const float* img = a.input + (size_t)g.b * a.C * hw;
    const int c0 = blockIdx.y * cpw, c1 = min(a.OD, c0 + cpw);
    int cur = -1;
    float ws = 0.0f, hs = 0.0f;
    for (int ctop = c0; ctop < c1; ++ctop) {
        const int cls = ctop / a.cec;
        if (cls != cur) {        // the sample geometry is shared by every channel of a class
            bin_start(a, g, n, cls, ph, pw, ws, hs);
            cur = cls;
        }
        const float* plane = img + (size_t)((ctop * a.G + gh) * a.G + gw) * hw;
        const size_t idx = ((size_t)n * a.OD + ctop) * PP + bin;
        float s0 = 0.0f, s1 = 0.0f, gv = 0.0f;
        int count = 0;
        if (GRAD) {
            const float cv = cnt[idx];
            if (cv <= 0.0f) {
                out0[2 * idx] = 0.0f;
                out0[2 * idx + 1] = 0.0f;
                continue;
            }
            gv = go[idx] / cv;
        }
        for (int ih = 0; ih < a.S; ++ih) {
            float h = hs + (float)ih * g.subh;
            if (outside(h, a.H)) continue;
            h = clamp_to(h, a.H);
            const int y0 = (int)floorf(h), y1 = (int)ceilf(h);
            const float dy = h - (float)y0;
            const float* r0 = plane + (size_t)y0 * a.W;
            const float* r1 = plane + (size_t)y1 * a.W;
            for (int iw = 0; iw < a.S; ++iw) {
                float w = ws + (float)iw * g.subw;
                if (outside(w, a.W)) continue;
                w = clamp_to(w, a.W);
                const int x0 = (int)floorf(w), x1 = (int)ceilf(w);
                const float dx = w - (float)x0;
                const float v00 = r0[x0], v01 = r1[x0], v10 = r0[x1], v11 = r1[x1];      // v<x><y>
                if (GRAD) {
                    float ddx = (v11 * dy + v10 * (1.0f - dy) - v01 * dy - v00 * (1.0f - dy)) * a.tstd * gv;
                    float ddy = (v11 * dx + v01 * (1.0f - dx) - v10 * dx - v00 * (1.0f - dx)) * a.tstd * gv;
                    s0 += ddx * g.rw;
                    s1 += ddy * g.rh;
                } else {
                    s0 += (1.0f - dx) * (1.0f - dy) * v00 + (1.0f - dx) * dy * v01 + dx * (1.0f - dy) * v10 +
                          dx * dy * v11;
                    ++count;
                }
            }
        }
        if (GRAD) {
            out0[2 * idx] = s0;
            out0[2 * idx + 1] = s1;
        } else {
            out0[idx] = count == 0 ? 0.0f : s0 / (float)count;
            out1[idx] = (float)count;
        }
    }
}

// grad_trans[n][cls][xy][part_h][part_w]: one wave per element.  Lane l adds the (channel of the class, bin) pairs
// l, l + 64, ... that belong to the part cell, in ascending order; the 64 lane sums then meet in the fixed xor tree.
__global__ __launch_bounds__(kWave) void psroi_offset_reduce_kernel(Psroi a, const float* __restrict__ partial,
                                                                   float* __restrict__ grad_trans) {
    const int pp = a.part * a.part, PP = a.P * a.P;
    const long long i = blockIdx.x;
    const int cell = (int)(i % pp), xy = (int)((i / pp) % 2), cls = (int)((i / (2 * pp)) % a.nc);
    const int n = (int)(i / ((long long)2 * pp * a.nc));
    const int cell_h = cell / a.part, cell_w = cell - cell_h * a.part;
    const float* p = partial + ((size_t)n * a.OD + (size_t)cls * a.cec) * PP * 2 + xy;
    float s = 0.0f;
    for (int e = threadIdx.x; e < a.cec * PP; e += kWave) {
        const int bin = e % PP, ph = bin / a.P, pw = bin - ph * a.P;
        if (a.part_of[ph] == cell_h && a.part_of[pw] == cell_w) s += p[2 * (size_t)e];
    }
    s = wave_sum(s);
    if (threadIdx.x == 0) grad_trans[i] = s;
}

// lists[b] = number of ROIs of image b; lists[B + b * N + k] = index of its k-th ROI (ascending)
__global__ __launch_bounds__(kWave) void psroi_roi_lists_kernel(const float* __restrict__ rois, int N, int B,
                                                                int* __restrict__ lists) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int* list = lists + B + (size_t)b * N;
    int total = 0;
    for (int base = 0; base < N; base += kWave) {
        const int i = base + lane;
        const bool mine = i < N && (int)rois[(size_t)i * 5] == b;
        const unsigned long long m = __ballot(mine);
        if (mine) list[total + __popcll(m & ((1ull << lane) - 1ull))] = i;
        total += __popcll(m);
    }
    if (lane == 0) lists[b] = total;
}

// One wave owns rows [r0, r1) of plane (b, c), held in LDS.  For a bin, the weight of its samples on pixel (y, x) is
// separable: (sum over valid iw of hat(clamp(w_iw) - x)) * (sum over valid ih of hat(clamp(h_ih) - y)), and
// count = #valid iw * #valid ih.  Per ROI the 64 lanes first prepare 64 bins (count, gradient, offsets, footprint); the
// bins that reach this tile are then taken one by one in bin order, the lanes spread over the footprint's pixels.
__global__ __launch_bounds__(kWave) void psroi_grad_input_kernel(Psroi a, const float* __restrict__ go,
                                                                 const float* __restrict__ cnt,
                                                                 const int* __restrict__ lists,
                                                                 float* __restrict__ grad_input, int acc, int TH) {
    extern __shared__ float tile[];
    const int lane = threadIdx.x;
    const int tiles = (a.H + TH - 1) / TH;
    const int plane = blockIdx.x / tiles, t = blockIdx.x - plane * tiles;
    const int b = plane / a.C, c = plane - b * a.C;
    const int r0 = t * TH, r1 = min(a.H, r0 + TH);
    const int ctop = c / (a.G * a.G), gh = (c / a.G) % a.G, gw = c % a.G;
    const int cls = ctop / a.cec;
    const int PP = a.P * a.P;
    const int npx = (r1 - r0) * a.W;
    for (int i = lane; i < npx; i += kWave) tile[i] = 0.0f;
    __syncthreads();
    const int nroi = lists[b];
    const int* list = lists + a.B + (size_t)b * a.N;
    for (int k = 0; k < nroi; ++k) {
        const int n = list[k];
        const RoiGeom g = roi_geom(a, n);
        for (int base = 0; base < PP; base += kWave) {
            const int bin = base + lane;
            bool live = false;
            float ws = 0.0f, hs = 0.0f, gv = 0.0f;
            int xlo = a.W, xhi = -1, ylo = a.H, yhi = -1;
            if (bin < PP) {
                const int ph = bin / a.P, pw = bin - ph * a.P;
                if (a.g_of[ph] == gh && a.g_of[pw] == gw) {
                    const size_t idx = ((size_t)n * a.OD + ctop) * PP + bin;
                    const float cv = cnt[idx];
                    if (cv > 0.0f) {
                        gv = go[idx] / cv;
                        bin_start(a, g, n, cls, ph, pw, ws, hs);
                        for (int s = 0; s < a.S; ++s) {
                            const float w = ws + (float)s * g.subw, h = hs + (float)s * g.subh;
                            if (!outside(w, a.W)) {
                                const float cw = clamp_to(w, a.W);
                                xlo = min(xlo, (int)floorf(cw));
                                xhi = max(xhi, (int)ceilf(cw));
                            }
                            if (!outside(h, a.H)) {
                                const float ch = clamp_to(h, a.H);
                                ylo = min(ylo, (int)floorf(ch));
                                yhi = max(yhi, (int)ceilf(ch));
                            }
                        }
                        ylo = max(ylo, r0);
                        yhi = min(yhi, r1 - 1);
                        live = xlo <= xhi && ylo <= yhi;
                    }
                }
            }
            unsigned long long m = __ballot(live);
            while (m) {
                const int j = __ffsll((long long)m) - 1;
                m &= m - 1ull;
                const float bws = __shfl(ws, j, kWave), bhs = __shfl(hs, j, kWave), bgv = __shfl(gv, j, kWave);
                const int bxlo = __shfl(xlo, j, kWave), bxhi = __shfl(xhi, j, kWave);
                const int bylo = __shfl(ylo, j, kWave), byhi = __shfl(yhi, j, kWave);
                const int fw = bxhi - bxlo + 1, fpx = fw * (byhi - bylo + 1);
                for (int i = lane; i < fpx; i += kWave) {
                    const int fy = i / fw;
                    const int x = bxlo + (i - fy * fw), y = bylo + fy;
                    float ax = 0.0f, ay = 0.0f;
                    for (int s = 0; s < a.S; ++s) {
                        const float w = bws + (float)s * g.subw, h = bhs + (float)s * g.subh;
                        if (!outside(w, a.W)) ax += fmaxf(0.0f, 1.0f - fabsf(clamp_to(w, a.W) - (float)x));
                        if (!outside(h, a.H)) ay += fmaxf(0.0f, 1.0f - fabsf(clamp_to(h, a.H) - (float)y));
                    }
                    tile[(y - r0) * a.W + x] += bgv * ax * ay;
                }
                __syncthreads();       // the next bin's footprint may hand this pixel to another lane
            }
        }
    }
    float* dst = grad_input + ((size_t)plane * a.H + r0) * a.W;
    for (int i = lane; i < npx; i += kWave) dst[i] = acc ? dst[i] + tile[i] : tile[i];
}

// geometry checks shared by the three entry points; fills the argument block
int fill(Psroi& a, const char* who, int B, int channels, int H, int W, int num_rois, int no_trans, float spatial_scale,
         int output_dim, int group_size, int pooled_size, int part_size, int sample_per_part, float trans_std,
         int num_classes) {
    CNUDA_REQUIRE(B > 0 && channels > 0 && H > 0 && W > 0 && num_rois >= 0, "%s: bad tensor geometry", who);
    CNUDA_REQUIRE(output_dim > 0 && group_size > 0 && pooled_size > 0 && part_size > 0 && sample_per_part > 0 &&
                      num_classes > 0,
                  "%s: output_dim, group_size, pooled_size, part_size, sample_per_part, num_classes must be positive",
                  who);
    CNUDA_REQUIRE(pooled_size <= kMaxPooled && part_size <= 255 && group_size <= 255 && output_dim <= (1 << 17),
                  "%s: pooled_size %d > %d (or part_size / group_size > 255, output_dim > 131072)", who, pooled_size,
                  kMaxPooled);
    CNUDA_REQUIRE((long long)output_dim * group_size * group_size == channels,
                  "%s: input has %d channels, output_dim * group_size^2 = %lld", who, channels,
                  (long long)output_dim * group_size * group_size);
    CNUDA_REQUIRE(!(no_trans && num_classes != 1), "%s: no_trans takes num_classes = 1", who);
    CNUDA_REQUIRE(output_dim % num_classes == 0, "%s: output_dim %d is not a multiple of num_classes %d", who,
                  output_dim, num_classes);
    CNUDA_REQUIRE(W <= kMaxTileFloats, "%s: map width %d > %d", who, W, kMaxTileFloats);
    CNUDA_REQUIRE((long long)num_rois * output_dim * pooled_size * pooled_size < (1ll << 31) &&
                      (long long)B * channels * H < (1ll << 31),
                  "%s: problem too large", who);
    a.B = B, a.C = channels, a.H = H, a.W = W, a.N = num_rois, a.no_trans = no_trans ? 1 : 0;
    a.OD = output_dim, a.G = group_size, a.P = pooled_size, a.part = part_size, a.S = sample_per_part;
    a.nc = num_classes, a.cec = output_dim / num_classes;
    a.scale = spatial_scale, a.tstd = trans_std;
    for (int p = 0; p < pooled_size; ++p) {
        // IEEE float, in the reference's operation order: int -> float, then / P * part, resp. * G / P
        volatile float q = (float)p / (float)pooled_size;
        q = q * (float)part_size;
        int cell = (int)floorf(q);
        volatile float r = (float)p * (float)group_size;
        r = r / (float)pooled_size;
        int grp = (int)floorf(r);
        cell = cell < part_size - 1 ? cell : part_size - 1;      // (never beyond the offset tensor)
        grp = grp < 0 ? 0 : (grp > group_size - 1 ? group_size - 1 : grp);
        a.part_of[p] = (unsigned char)cell;
        a.g_of[p] = (unsigned char)grp;
    }
    return 0;
}

// the batch indices live on the device: read them back (one small copy, one stream synchronisation) so that a ROI that
// names no image is an error code and not an out-of-bounds read
int check_rois(const char* who, const float* rois, int N, int B, hipStream_t st) {
    if (N == 0) return 0;
    std::vector<float> h((size_t)N * 5);
    hipError_t e = hipMemcpyAsync(h.data(), rois, sizeof(float) * h.size(), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        set_error("%s: reading the ROIs back: %s", who, hipGetErrorString(e));
        return (int)e;
    }
    for (int i = 0; i < N; ++i) {
        const float v = h[(size_t)i * 5];
        CNUDA_REQUIRE(v > -1.0f && v < (float)B, "%s: roi %d names batch index %g, the input has %d images", who, i,
                      (double)v, B);
    }
    return 0;
}

int channels_per_wave(const Psroi& a) {
    const long long waves8 = (long long)a.N * ((a.P * a.P + kWave - 1) / kWave) * ((a.OD + 7) / 8);
    return waves8 >= 512 ? 8 : 4;
}

size_t lists_bytes(int B, int N) { return (((size_t)B + (size_t)B * N) * sizeof(int) + 255) / 256 * 256; }

}  // namespace
}  // namespace cnuda

using namespace cnuda;

extern "C" size_t cnuda_dcn_v2_psroi_pooling_workspace_bytes(int B, int num_rois, int output_dim, int pooled_size) {
    if (B <= 0 || num_rois < 0 || output_dim <= 0 || pooled_size <= 0) return 0;
    return lists_bytes(B, num_rois) + (size_t)2 * num_rois * output_dim * pooled_size * pooled_size * sizeof(float) +
           256;
}

extern "C" int cnuda_dcn_v2_psroi_pooling_forward(const float* input, const float* rois, const float* trans,
                                                  float* output, float* output_count, int B, int channels, int H,
                                                  int W, int num_rois, int no_trans, float spatial_scale,
                                                  int output_dim, int group_size, int pooled_size, int part_size,
                                                  int sample_per_part, float trans_std, int num_classes,
                                                  cnuda_stream_t stream) {
    const char* who = "cnuda_dcn_v2_psroi_pooling_forward";
    Psroi a;
    if (int rc = fill(a, who, B, channels, H, W, num_rois, no_trans, spatial_scale, output_dim, group_size,
                      pooled_size, part_size, sample_per_part, trans_std, num_classes))
        return rc;
    if (num_rois == 0) return 0;
    CNUDA_REQUIRE(input && rois && output && output_count && (no_trans || trans), "%s: null pointer", who);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = check_rois(who, rois, num_rois, B, st)) return rc;
    a.input = input, a.rois = rois, a.trans = no_trans ? nullptr : trans;
    const int cpw = channels_per_wave(a);
    const dim3 grid(num_rois * ceil_div(pooled_size * pooled_size, kWave), ceil_div(output_dim, cpw));
    CNUDA_LAUNCH(psroi_bins_kernel<false>, grid, dim3(kWave), 0, st, a, cpw, (const float*)nullptr,
                 (const float*)nullptr, output, output_count);
    return check_launch(who);
}

extern "C" int cnuda_dcn_v2_psroi_pooling_backward(const float* grad_output, const float* input, const float* rois,
                                                   const float* trans, const float* output_count, float* grad_input,
                                                   int acc, float* grad_trans, int B, int channels, int H, int W,
                                                   int num_rois, int no_trans, float spatial_scale, int output_dim,
                                                   int group_size, int pooled_size, int part_size,
                                                   int sample_per_part, float trans_std, int num_classes,
                                                   void* workspace, size_t workspace_bytes, cnuda_stream_t stream) {
    const char* who = "cnuda_dcn_v2_psroi_pooling_backward";
    Psroi a;
    if (int rc = fill(a, who, B, channels, H, W, num_rois, no_trans, spatial_scale, output_dim, group_size,
                      pooled_size, part_size, sample_per_part, trans_std, num_classes))
        return rc;
    CNUDA_REQUIRE(input && grad_input && (num_rois == 0 || (grad_output && rois && output_count)) &&
                      (no_trans || num_rois == 0 || (trans && grad_trans)),
                  "%s: null pointer", who);
    CNUDA_REQUIRE(workspace &&
                      workspace_bytes >= cnuda_dcn_v2_psroi_pooling_workspace_bytes(B, num_rois, output_dim, pooled_size),
                  "%s: workspace", who);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = check_rois(who, rois, num_rois, B, st)) return rc;
    a.input = input, a.rois = rois, a.trans = no_trans ? nullptr : trans;
    int* lists = (int*)workspace;
    float* partial = (float*)((char*)workspace + lists_bytes(B, num_rois));

    // grad_input: rows per tile from the LDS budget, fewer when the planes alone do not fill the device
    int TH = kMaxTileFloats / W;
    TH = TH < H ? TH : H;
    const long long planes = (long long)B * channels;
    const int want_tiles = ceil_div(1024, planes);
    const int rows = ceil_div(H, want_tiles) > 8 ? ceil_div(H, want_tiles) : 8;
    TH = TH < rows ? TH : rows;
    const long long blocks = planes * ceil_div(H, TH);
    CNUDA_REQUIRE(blocks < (1ll << 31), "%s: problem too large", who);
    CNUDA_LAUNCH(psroi_roi_lists_kernel, dim3(B), dim3(kWave), 0, st, rois, num_rois, B, lists);
    CNUDA_LAUNCH(psroi_grad_input_kernel, dim3((unsigned)blocks), dim3(kWave), sizeof(float) * TH * W, st, a,
                 grad_output, output_count, (const int*)lists, grad_input, acc ? 1 : 0, TH);
    if (!no_trans && num_rois > 0) {
        const int cpw = channels_per_wave(a);
        const dim3 grid(num_rois * ceil_div(pooled_size * pooled_size, kWave), ceil_div(output_dim, cpw));
        CNUDA_LAUNCH(psroi_bins_kernel<true>, grid, dim3(kWave), 0, st, a, cpw, grad_output, output_count, partial,
                     (float*)nullptr);
        const long long total = (long long)num_rois * num_classes * 2 * part_size * part_size;
        CNUDA_REQUIRE(total < (1ll << 31), "%s: problem too large", who);
        CNUDA_LAUNCH(psroi_offset_reduce_kernel, dim3((unsigned)total), dim3(kWave), 0, st, a, (const float*)partial,
                     grad_trans);
    }
    return check_launch(who);
}
