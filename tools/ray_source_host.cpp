// ray_source_host -- a stand-alone host program over octpt_ray_source_rays, for sanitizer runs of the
// host entry (tests/test_ray_source_cpu.py compiles it with octpt_host.cpp under -fsanitize=address,undefined).
// Reads cases from the file named by argv[1] and prints each case's rays:
//   in:  width height rays_per_pixel seed samples, then eye[3] direction[3] up[3] fov as C99 hex floats, then the list's
//        6 * width * height * rays_per_pixel floats as hex words (any bit pattern: NaN and infinities included)
//   out: one line per case: for samples 0 .. samples-1 of every pixel in image order the 6 ray words, then the RNG
//        states, as hex
// Every case is also run through the refusals, which must write nothing.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/octpt.h"

static int fail(const char *what) {
    std::fprintf(stderr, "ray_source_host: %s\n", what);
    return 1;
}

int main(int argc, char **argv) {
    if (argc != 2) return fail("usage: ray_source_host CASES");
    FILE *f = std::fopen(argv[1], "r");
    if (!f) return fail("cannot open the cases file");
    unsigned W, H, R, seed, S;
    while (std::fscanf(f, "%u %u %u %u %u", &W, &H, &R, &seed, &S) == 5) {
        float v[10];
        for (float &x : v)
            if (std::fscanf(f, "%f", &x) != 1) return fail("bad camera row");
        octpt_camera cam{};
        std::memcpy(cam.eye, v, 12);
        std::memcpy(cam.direction, v + 3, 12);
        std::memcpy(cam.up, v + 6, 12);
        cam.fov = v[9];
        // exact-size arrays: a read or write past any of them is the sanitizer's to report
        std::vector<float> list((size_t)6 * W * H * R);
        for (float &x : list) {
            unsigned u;
            if (std::fscanf(f, "%x", &u) != 1) return fail("bad list word");
            std::memcpy(&x, &u, 4);
        }
        const size_t n = (size_t)W * H * S;
        std::vector<uint32_t> xys(3 * n), state(n);
        std::vector<float> rays(6 * n);
        size_t i = 0;
        for (uint32_t s = 0; s < S; ++s)
            for (uint32_t y = 0; y < H; ++y)
                for (uint32_t x = 0; x < W; ++x, ++i) {
                    xys[3 * i] = x;
                    xys[3 * i + 1] = y;
                    xys[3 * i + 2] = s;
                }
        // the refusals first, into marked arrays: nothing may be written
        const float mark = 123.25f;
        for (float &x : rays) x = mark;
        for (uint32_t &s : state) s = 0xA5A5A5A5u;
        for (int bad = 0; bad < 7; ++bad) {
            octpt_camera c = cam;
            std::vector<uint32_t> q = xys;
            uint32_t w = W, h = H, r = R;
            const float *l = list.data();
            if (bad == 0) r = 0u;
            if (bad == 1) w = 0u;
            if (bad == 2) w = 1u << 15, h = 1u << 14;  // 2^29 rays (checked before the list is read)
            if (bad == 3) c.fov = 0.0f;
            if (bad == 4) q[3 * (n - 1)] = W;  // the last row's pixel lies outside the frame
            if (bad == 5) q[3 * (n - 1) + 1] = H;
            if (bad == 6) l = nullptr;
            if (octpt_ray_source_rays(&c, l, w, h, r, seed, q.data(), (uint32_t)n, rays.data(), state.data()) !=
                OCTPT_ERR_INVALID_ARG)
                return fail("a refusal returned another status");
        }
        for (float x : rays)
            if (x != mark) return fail("a refused call wrote rays");
        for (uint32_t s : state)
            if (s != 0xA5A5A5A5u) return fail("a refused call wrote states");
        if (octpt_ray_source_rays(&cam, list.data(), W, H, R, seed, xys.data(), (uint32_t)n, rays.data(), nullptr) != OCTPT_OK)
            return fail("the case was refused");
        std::vector<float> again(6 * n);
        if (octpt_ray_source_rays(&cam, list.data(), W, H, R, seed, xys.data(), (uint32_t)n, again.data(), state.data()) !=
            OCTPT_OK)
            return fail("the case was refused");
        if (std::memcmp(rays.data(), again.data(), rays.size() * sizeof(float)) != 0)
            return fail("the rays depend on the state pointer");
        for (float x : rays) {
            uint32_t u;
            std::memcpy(&u, &x, 4);
            std::printf("%x ", u);
        }
        for (uint32_t s : state) std::printf("%x ", s);
        std::printf("\n");
    }
    std::fclose(f);
    return 0;
}
