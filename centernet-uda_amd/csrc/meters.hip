// Running statistics of a training loop on the device (utils/helper.py DeviceMeters): the reference's driver does
//   m.update(stats[k].item(), n)     ->   m.val = v; m.sum += v * n; m.count += n            (train.py:162-166)
// once per statistic and step, and every .item() is a blocking read-back.  Here the S loss scalars of a step stay
// where the loss kernels left them and ONE launch folds them into the meters' device arrays; the host reads the arrays
// once per epoch.
//
// The S device pointers travel by value in the kernel arguments (a 256-byte record): no upload, nothing for the host
// to keep alive.  One 64-lane workgroup; lane i < S owns meter i alone, so plain loads and stores do, without atomics.
// The product and the sum are two separately rounded float64 operations (__dmul_rn / __dadd_rn, and the build has
// -ffp-contract=off): the IEEE sequence of AverageMeter.update(float(v), n) in Python, hence bit-identical sums.
#include "common.h"

namespace cnuda {
namespace {

constexpr int kMeterSlots = 32;

struct MeterPointers { const float* value[kMeterSlots]; };

__global__ __launch_bounds__(64) void meter_update_kernel(MeterPointers src, int S, double n, double* __restrict__ sum,
                                                          double* __restrict__ count, float* __restrict__ last) {
    const int lane = threadIdx.x;
    if (lane >= S) return;
    // a select chain over the argument record instead of a lane-indexed read of it (which would copy the record to
    // scratch memory first)
    const float* p = src.value[0];
#pragma unroll
    for (int i = 1; i < kMeterSlots; ++i)
        if (lane == i) p = src.value[i];
    const float v = *p;
    sum[lane] = __dadd_rn(sum[lane], __dmul_rn((double)v, n));
    count[lane] = __dadd_rn(count[lane], n);
    last[lane] = v;
}

}  // namespace
}  // namespace cnuda

using namespace cnuda;

extern "C" int cnuda_meter_update(const float* const* values, int S, double n, double* sum, double* count, float* last,
                                  cnuda_stream_t stream) {
    CNUDA_REQUIRE(values && sum && count && last, "cnuda_meter_update: null pointer");
    CNUDA_REQUIRE(S >= 1 && S <= kMeterSlots, "cnuda_meter_update: 1 to %d values per launch, got %d", kMeterSlots, S);
    CNUDA_REQUIRE(n >= 0.0, "cnuda_meter_update: the weight must not be negative (or NaN), got %g", n);
    CNUDA_REQUIRE((((uintptr_t)sum | (uintptr_t)count) & 7) == 0 && ((uintptr_t)last & 3) == 0,
                  "cnuda_meter_update: sum / count must be 8-byte and last 4-byte aligned");
    MeterPointers src;
    for (int i = 0; i < kMeterSlots; ++i) {
        src.value[i] = i < S ? values[i] : nullptr;
        CNUDA_REQUIRE(i >= S || (src.value[i] && ((uintptr_t)src.value[i] & 3) == 0),
                      "cnuda_meter_update: value %d is a null or misaligned pointer", i);
    }
    CNUDA_LAUNCH(meter_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, src, S, n, sum, count, last);
    return check_launch("cnuda_meter_update");
}
