// Detection previews on the GPU: what utils/visualize.py:23-49 of the reference paints with one imgaug / cv2 / PIL call
// per object on a host copy of the float batch -- the denormalised image twice, prediction panel left and ground-truth
// panel right, with boxes, rotated outlines, label bars, text and keypoints blended over it -- as ONE launch that reads
// the resident `input` and writes the finished uint8 picture (DESIGN.md section 23 has the pixel rules).
//
// A gather: one workgroup owns a 64 x 16 tile of one rendered image's [H, 2W] output plane triple and walks that
// image's primitive range in chunks of kChunk records, one record per thread.  Each thread clamps its record, derives
// the bounding box of its pixel set and tests it against the tile and the panel; survivors are compacted IN LIST ORDER
// into LDS (a wave64 ballot gives the rank inside the wave, the four waves' counts the wave's offset); then every
// thread applies the compacted records in order to the four consecutive pixels of one row that it keeps in registers.
// No atomics, no floating-point reduction: the result is bit-stable.  Tiles without primitives (most of a picture)
// only denormalise.  The base pixel is read as one 16-byte load per channel where W % 4 == 0 and stored as one dword
// per channel plane where 2W % 4 == 0; other widths, and the up to three pixels behind the last whole group of a row,
// take scalar loads and byte stores.
#include "common.h"

namespace cnuda {
namespace {

constexpr int kChunk = CNUDA_RENDER_CHUNK;       // records per pass = threads per workgroup
constexpr int kRec = CNUDA_RENDER_RECORD;        // int32 words per record
constexpr int kTileW = 64, kTileH = 16;          // 16 groups of four pixels x 16 rows = 256 threads
constexpr int kCoordMax = 32767, kCoordMin = -32768, kThickMax = 1024;
static_assert(kChunk == kTileW / 4 * kTileH && kChunk % kWave == 0 && kRec == 16, "render tile / record layout");

enum { kRing = 0, kFill = 1, kQuad = 2, kGlyph = 3 };

struct Denorm3 { float mean[3], std[3]; };

// what the apply loop reads from LDS: the clamped record plus the bounding box of its pixel set (panel-local, inclusive)
struct __align__(16) Prim {
    int kind, panel, color, alpha;     // colour r | g << 8 | b << 16; alpha: float bits
    int t, g0, g1, g2;                 // t: thickness (RING, QUAD) or glyph index (GLYPH); g0..g7: geometry
    int g3, g4, g5, g6;
    int g7, bx1, by1, bx2;
    int by2, pad0, pad1, pad2;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// 4 d^2 <= t^2 for the distance d from X to the segment PQ, exactly (header: the QUAD rule).  |coordinates| <= 2^15 + 2^13
// and t <= 2^10: every product below fits int64 except cross^2, which is only formed when |cross| < 2^27 -- beyond that
// 4 cross^2 >= 2^56 exceeds t^2 L <= 2^20 * 2^34 and the answer is "outside" without it.
__device__ __forceinline__ bool near_segment(int x, int y, int px, int py, int qx, int qy, long long tt) {
    const long long ex = qx - px, ey = qy - py, wx = x - px, wy = y - py;
    const long long L = ex * ex + ey * ey, s = wx * ex + wy * ey;
    if (s <= 0) return 4 * (wx * wx + wy * wy) <= tt;
    if (s >= L) {
        const long long ux = x - qx, uy = y - qy;
        return 4 * (ux * ux + uy * uy) <= tt;
    }
    long long cross = wx * ey - wy * ex;
    if (cross < 0) cross = -cross;
    if (cross >= (1ll << 27)) return false;
    return 4 * cross * cross <= tt * L;
}

__device__ __forceinline__ float blend1(float v, float a, float c) {
    const float r = rintf(v + a * (c - v));            // one subtract, one multiply, one add (no contraction), half-even
    return fminf(fmaxf(r, 0.0f), 255.0f);              // a byte again (alpha outside [0, 1] cannot leave the range)
}

__global__ __launch_bounds__(kChunk) void render_detections_kernel(
        const float* __restrict__ input, const int* __restrict__ index, const int* __restrict__ prims,
        const int* __restrict__ first, const unsigned char* __restrict__ atlas, unsigned char* __restrict__ out,
        int B, int H, int W, int N, int G, int gh, int gw, Denorm3 dn, int wide_in, int wide_out) {
    __shared__ Prim s_prim[kChunk];
    __shared__ int s_count[kChunk / kWave];

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int img = blockIdx.z, W2 = 2 * W;
    const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
    const int ox0 = tx0 + (tid & 15) * 4, y = ty0 + (tid >> 4);
    const long long HW = (long long)H * W;

    // ---- base pixels: four consecutive output columns of row y; column ox belongs to panel ox >= W, local x = ox - panel * W
    int src = index[img];
    const bool have_src = src >= 0 && src < B;         // an index that names no image renders over black
    if (!have_src) src = 0;
    const float* in0 = input + (long long)src * 3 * HW;
    float v[3][4];
    int lx[4], pan[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int ox = ox0 + p;
        pan[p] = ox >= W ? 1 : 0;
        lx[p] = ox - pan[p] * W;
    }
    const bool row_ok = y < H;
    if (row_ok && have_src && wide_in && ox0 + 3 < W2) {          // W % 4 == 0: the four pixels share a panel, 16-byte aligned
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float4 q = *reinterpret_cast<const float4*>(in0 + c * HW + (long long)y * W + lx[0]);
            v[c][0] = q.x, v[c][1] = q.y, v[c][2] = q.z, v[c][3] = q.w;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int p = 0; p < 4; ++p)
                v[c][p] = (row_ok && have_src && ox0 + p < W2) ? in0[c * HW + (long long)y * W + lx[p]] : 0.0f;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const float f = (v[c][p] * dn.std[c] + dn.mean[c]) * 255.0f;
            v[c][p] = have_src ? (float)(int)fminf(fmaxf(f, 0.0f), 255.0f) : 0.0f;     // clamp, then truncate
        }

    // ---- this image's primitives, kChunk at a time
    int begin = first[img], end = first[img + 1];
    begin = begin < 0 ? 0 : begin;
    end = end > N ? N : end;
    for (int base = begin; base < end; base += kChunk) {
        const int idx = base + tid;
        Prim r;
        bool keep = false;
        if (idx < end) {
            const int4* rec = reinterpret_cast<const int4*>(prims + (long long)idx * kRec);
            const int4 a = rec[0], b = rec[1], c = rec[2], d = rec[3];
            r.kind = a.x, r.panel = a.y, r.color = a.z, r.alpha = a.w;
            r.t = b.x;
            r.g0 = clampi(b.y, kCoordMin, kCoordMax), r.g1 = clampi(b.z, kCoordMin, kCoordMax);
            r.g2 = clampi(b.w, kCoordMin, kCoordMax), r.g3 = clampi(c.x, kCoordMin, kCoordMax);
            r.g4 = clampi(c.y, kCoordMin, kCoordMax), r.g5 = clampi(c.z, kCoordMin, kCoordMax);
            r.g6 = clampi(c.w, kCoordMin, kCoordMax), r.g7 = clampi(d.x, kCoordMin, kCoordMax);
            r.pad0 = r.pad1 = r.pad2 = 0;
            bool known = true;
            if (r.kind == kFill) {
                r.bx1 = r.g0, r.by1 = r.g1, r.bx2 = r.g2, r.by2 = r.g3;
            } else if (r.kind == kRing) {
                r.t = clampi(r.t, 0, kThickMax);
                r.bx1 = r.g0 - r.t + 1, r.by1 = r.g1 - r.t + 1, r.bx2 = r.g2 + r.t - 1, r.by2 = r.g3 + r.t - 1;
            } else if (r.kind == kQuad) {
                r.t = clampi(r.t, 0, kThickMax);
                const int h = (r.t + 1) / 2;                       // 4 d^2 <= t^2  =>  |dx|, |dy| <= t / 2
                r.bx1 = min(min(r.g0, r.g2), min(r.g4, r.g6)) - h, r.bx2 = max(max(r.g0, r.g2), max(r.g4, r.g6)) + h;
                r.by1 = min(min(r.g1, r.g3), min(r.g5, r.g7)) - h, r.by2 = max(max(r.g1, r.g3), max(r.g5, r.g7)) + h;
            } else if (r.kind == kGlyph) {
                known = r.t >= 0 && r.t < G;                       // a glyph the atlas does not hold is skipped
                r.bx1 = r.g0, r.by1 = r.g1, r.bx2 = r.g0 + gw - 1, r.by2 = r.g1 + gh - 1;
            } else {
                known = false;
                r.bx1 = r.by1 = 0, r.bx2 = r.by2 = -1;
            }
            // the tile sees the box clipped to the primitive's own panel, shifted into output columns
            const int shift = r.panel == 1 ? W : 0;
            const int cx1 = max(r.bx1, 0) + shift, cx2 = min(r.bx2, W - 1) + shift;
            keep = known && (r.panel == 0 || r.panel == 1) && max(r.bx1, 0) <= min(r.bx2, W - 1) && cx1 <= tx0 + kTileW - 1
                   && cx2 >= tx0 && r.by1 <= ty0 + kTileH - 1 && r.by2 >= ty0 && r.by1 <= r.by2;
        }
        const unsigned long long vote = __ballot(keep);
        if (lane == 0) s_count[wave] = __popcll(vote);
        __syncthreads();
        int slot = __popcll(vote & ((1ull << lane) - 1)), total = 0;
#pragma unroll
        for (int w = 0; w < kChunk / kWave; ++w) {
            const int n = s_count[w];
            slot += w < wave ? n : 0;
            total += n;
        }
        if (keep) s_prim[slot] = r;
        __syncthreads();

        for (int k = 0; k < total; ++k) {
            const Prim& q = s_prim[k];
            const int kind = q.kind, ppanel = q.panel;
            const float cr = (float)(q.color & 255), cg = (float)((q.color >> 8) & 255), cb = (float)((q.color >> 16) & 255);
            const float alpha = __int_as_float(q.alpha);
            if (y < q.by1 || y > q.by2) continue;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int x = lx[p];
                if (pan[p] != ppanel || x < q.bx1 || x > q.bx2) continue;
                float a = alpha;
                if (kind == kRing) {
                    if (q.g0 < x && x < q.g2 && q.g1 < y && y < q.g3) continue;
                } else if (kind == kQuad) {
                    const long long tt = (long long)q.t * q.t;
                    if (!(near_segment(x, y, q.g0, q.g1, q.g2, q.g3, tt) || near_segment(x, y, q.g2, q.g3, q.g4, q.g5, tt)
                          || near_segment(x, y, q.g4, q.g5, q.g6, q.g7, tt) || near_segment(x, y, q.g6, q.g7, q.g0, q.g1, tt)))
                        continue;
                } else if (kind == kGlyph) {
                    a = (float)atlas[((long long)q.t * gh + (y - q.g1)) * gw + (x - q.g0)] / 255.0f;
                }
                v[0][p] = blend1(v[0][p], a, cr);
                v[1][p] = blend1(v[1][p], a, cg);
                v[2][p] = blend1(v[2][p], a, cb);
            }
        }
        __syncthreads();                                           // the next chunk overwrites s_prim / s_count
    }

    // ---- store: one dword per channel plane, bytes where the row pitch or the row's end does not allow it
    if (!row_ok || ox0 >= W2) return;
    unsigned char* o0 = out + (long long)img * 3 * H * W2 + (long long)y * W2 + ox0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        unsigned char* o = o0 + (long long)c * H * W2;
        if (wide_out && ox0 + 3 < W2) {
            *reinterpret_cast<uint32_t*>(o) = (uint32_t)v[c][0] | (uint32_t)v[c][1] << 8 | (uint32_t)v[c][2] << 16
                                              | (uint32_t)v[c][3] << 24;
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (ox0 + p < W2) o[p] = (unsigned char)v[c][p];
        }
    }
}

}  // namespace
}  // namespace cnuda

using namespace cnuda;

extern "C" int cnuda_render_detections(const float* input, const int* index, const int* prims, const int* first,
                                       const unsigned char* atlas, unsigned char* out, int B, int n, int H, int W,
                                       int N, int G, int gh, int gw, float mean0, float mean1, float mean2,
                                       float std0, float std1, float std2, cnuda_stream_t stream) {
    CNUDA_REQUIRE(input && index && first && out, "cnuda_render_detections: null pointer");
    CNUDA_REQUIRE(B > 0 && n > 0 && n <= 65535 && H > 0 && W > 0, "cnuda_render_detections: bad sizes");
    CNUDA_REQUIRE(H <= 8192 && W <= 8192, "cnuda_render_detections: H and W must not exceed 8192");
    CNUDA_REQUIRE(N >= 0 && N <= (1 << 26) && (N == 0 || prims), "cnuda_render_detections: bad primitive list");
    CNUDA_REQUIRE(G >= 0 && G <= 65536 && (G == 0 || (atlas && gh > 0 && gw > 0 && gh <= 256 && gw <= 256)),
                  "cnuda_render_detections: bad glyph atlas");
    CNUDA_REQUIRE((((uintptr_t)input | (uintptr_t)index | (uintptr_t)first) & 3) == 0 && ((uintptr_t)prims & 15) == 0,
                  "cnuda_render_detections: input, index and first must be 4-byte and prims 16-byte aligned");
    const Denorm3 dn = {{mean0, mean1, mean2}, {std0, std1, std2}};
    const int wide_in = (W % 4 == 0) && ((uintptr_t)input & 15) == 0;
    const int wide_out = (W % 2 == 0) && ((uintptr_t)out & 3) == 0;          // 2W % 4 == 0
    const dim3 grid(ceil_div(2 * W, kTileW), ceil_div(H, kTileH), n);
    hipStream_t st = (hipStream_t)stream;
    CNUDA_LAUNCH(render_detections_kernel, grid, dim3(kChunk), 0, st, input, index, prims, first, atlas, out, B, H, W,
                 N, G, gh, gw, dn, wide_in, wide_out);
    return check_launch("cnuda_render_detections");
}
