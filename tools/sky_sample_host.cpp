// tools/sky_sample_host.cpp -- the host builder and the host sample of the sky map's distribution (DESIGN.md C43:
// octpt_build_sky_distribution, octpt_sky_sample) in a program of its own, for a sanitizer build:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       -D__HIP_PLATFORM_AMD__ -I$ROCM_PATH/include tools/sky_sample_host.cpp octree_pathtracing_amd/csrc/octpt_host.cpp
// It runs both over the edge maps -- 1 x 1, 5 x 1, an all-black map, a map of FLT_MAX, one of NaN, negative and infinite
// texels, one bright texel -- into arrays of exactly the size the calls may write, with draws that include 0 and the
// largest float below 1, checks every picked texel and every pdf, and prints one line per map: width height total and
// a checksum of the samples.  tests/test_sky_sample_cpu.py builds and runs it and compares the lines with the library's.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/octpt.h"

namespace {

struct Map {
    uint32_t w, h;
    std::vector<float> texels;  // w * h * 4
};

Map constant(uint32_t w, uint32_t h, float v) {
    Map m{w, h, std::vector<float>((size_t)w * h * 4u, v)};
    return m;
}

uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

int run(const Map &m, float yaw) {
    const size_t n = (size_t)m.w * m.h;
    std::vector<uint64_t> row(m.h);
    std::vector<uint32_t> col(n);
    if (octpt_build_sky_distribution(m.texels.data(), m.w, m.h, row.data(), col.data()) != OCTPT_OK) return 1;
    const uint64_t total = row[m.h - 1u];
    octpt_sky_distribution_arrays a{};
    a.row_cdf = row.data();
    a.row_cdf_capacity = m.h;
    a.col_cdf = col.data();
    a.col_cdf_capacity = n;
    a.width = m.w;
    a.height = m.h;
    octpt_sky sky{};
    sky.mode = OCTPT_SKY_MAP;
    sky.scale = 1.0f;
    sky.yaw = yaw;
    sky.width = m.w;
    sky.height = m.h;
    const uint32_t N = 1024u;
    std::vector<float> u((size_t)N * 4u), out((size_t)N * 8u);
    uint32_t s = 12345u + m.w * 31u + m.h;
    const float below_one = std::nextafter(1.0f, 0.0f);
    for (size_t i = 0; i < u.size(); ++i) {
        const uint32_t r = lcg(s);
        u[i] = (r >> 28) == 0u ? 0.0f : (r >> 28) == 1u ? below_one : (float)(r >> 8) * (1.0f / 16777216.0f);
    }
    if (octpt_sky_sample(&a, &sky, N, u.data(), out.data()) != OCTPT_OK) return 2;
    uint32_t sum = 0u;
    for (uint32_t i = 0; i < N; ++i) {
        uint32_t w[4];
        std::memcpy(w, &out[8u * (size_t)i + 4u], 16);
        const float pdf = out[8u * (size_t)i + 3u];
        if (w[3] > 1u) return 3;
        if (w[3] == 1u) {
            if (total == 0u || w[0] >= m.w || w[1] >= m.h || w[2] == 0u || w[2] > 65536u) return 4;
            if (!(pdf > 0.0f) || !(pdf < std::numeric_limits<float>::infinity())) return 5;
            const float *d = &out[8u * (size_t)i];
            const float len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            if (!(std::fabs(len - 1.0f) < 1e-5f)) return 6;
        } else if (pdf != 0.0f) {
            return 7;
        }
        for (int k = 0; k < 8; ++k) {
            uint32_t b;
            std::memcpy(&b, &out[8u * (size_t)i + k], 4);
            sum = sum * 31u + b;
        }
    }
    std::printf("%u %u %llu %08x\n", m.w, m.h, (unsigned long long)total, sum);
    return 0;
}

}  // namespace

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<Map> maps;
    maps.push_back(constant(1, 1, 0.75f));
    maps.push_back(constant(5, 1, 0.5f));
    maps.back().texels[4u * 3u + 1u] = 9.0f;
    maps.push_back(constant(8, 4, 0.0f));  // all black: total 0, no sample
    maps.push_back(constant(8, 4, FLT_MAX));
    Map odd = constant(33, 17, 0.25f);
    odd.texels[0] = nan;
    odd.texels[5] = -3.0f;
    odd.texels[4u * 40u] = inf;
    odd.texels[4u * 100u + 2u] = FLT_MAX;
    maps.push_back(odd);
    Map bright = constant(32, 16, 0.0f);
    bright.texels[4u * (4u * 32u + 7u) + 1u] = 2000.0f;
    maps.push_back(bright);
    for (const Map &m : maps)
        for (float yaw : {0.0f, 100.0f}) {
            const int e = run(m, yaw);
            if (e) {
                std::fprintf(stderr, "sky_sample_host: check %d failed on a %u x %u map\n", e, m.w, m.h);
                return 1;
            }
        }
    // the refusals: nothing is written
    uint64_t r1 = 7;
    uint32_t c1 = 7;
    const float t[4] = {1, 1, 1, 1};
    if (octpt_build_sky_distribution(t, 0, 1, &r1, &c1) != OCTPT_ERR_INVALID_ARG) return 1;
    if (octpt_build_sky_distribution(t, 32769, 1, &r1, &c1) != OCTPT_ERR_UNSUPPORTED) return 1;
    if (octpt_build_sky_distribution(nullptr, 1, 1, &r1, &c1) != OCTPT_ERR_INVALID_ARG) return 1;
    if (r1 != 7 || c1 != 7) return 1;
    std::printf("refusals ok\n");
    return 0;
}
