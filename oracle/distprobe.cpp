// Golden-answer harness for the DISTANCE functions alone, linked against the
// reference objects in oracle/_ref.
// Usage: distprobe <pairs.bin> <out.bin>
// pairs.bin: [int32 valuetype (0 float, 1 int8)][int32 ndims][int32 ppd]
//            [int32 dims[ndims]], then per dim, per pair: x[dim] y[dim]
// out.bin:   per dim, per pair: {float L2, float Cosine}, each the value of
//            COMMON::DistanceUtils::ComputeDistance<T> on those bytes.
// Prints "instruction_set <name>": the family of the functions that
// DistanceCalcSelector (DistanceUtils.h:119) returned on this machine.
#include "inc/Core/Common/DistanceUtils.h"
#include <cstdint>
#include <cstdio>
#include <vector>

using namespace SPTAG;
using namespace SPTAG::COMMON;

template <typename T>
static int run(FILE* in, FILE* out, int32_t ndims, int32_t ppd)
{
    std::vector<int32_t> dims(ndims);
    if (fread(dims.data(), 4, ndims, in) != (size_t)ndims) return 1;
    for (int32_t d : dims) {
        std::vector<T> x(d), y(d);
        for (int p = 0; p < ppd; p++) {
            if (fread(x.data(), sizeof(T), d, in) != (size_t)d) return 1;
            if (fread(y.data(), sizeof(T), d, in) != (size_t)d) return 1;
            float r[2];
            r[0] = DistanceUtils::ComputeDistance<T>(x.data(), y.data(), d, DistCalcMethod::L2);
            r[1] = DistanceUtils::ComputeDistance<T>(x.data(), y.data(), d, DistCalcMethod::Cosine);
            fwrite(r, 4, 2, out);
        }
    }
    return 0;
}

// Names the functions the selector itself hands out, the ones
// ComputeDistance calls: both metrics must have come from the same family.
template <typename T>
static const char* selected()
{
    typedef DistanceCalcReturn<T> Fn;
    const Fn l2 = DistanceCalcSelector<T>(DistCalcMethod::L2);
    const Fn cs = DistanceCalcSelector<T>(DistCalcMethod::Cosine);
    const struct { const char* name; Fn l2, cs; } family[] = {
        {"AVX512", &DistanceUtils::ComputeL2Distance_AVX512, &DistanceUtils::ComputeCosineDistance_AVX512},
        {"AVX", &DistanceUtils::ComputeL2Distance_AVX, &DistanceUtils::ComputeCosineDistance_AVX},
        {"SSE", &DistanceUtils::ComputeL2Distance_SSE, &DistanceUtils::ComputeCosineDistance_SSE},
        {"scalar", &DistanceUtils::ComputeL2Distance<T>, &DistanceUtils::ComputeCosineDistance<T>},
    };
    for (const auto& f : family)
        if (l2 == f.l2 && cs == f.cs) return f.name;
    return "mixed";
}

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "args\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 1;
    int32_t h[3];
    if (fread(h, 4, 3, in) != 3) return 1;
    int rc = h[0] == 0 ? run<float>(in, out, h[1], h[2])
                       : run<std::int8_t>(in, out, h[1], h[2]);
    fclose(in);
    fclose(out);
    printf("instruction_set %s\n", h[0] == 0 ? selected<float>() : selected<std::int8_t>());
    return rc;
}
