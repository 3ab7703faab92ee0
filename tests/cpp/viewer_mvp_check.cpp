// viewerMvp of ifx_host.hpp for tests/test_viewer_rule_cpu.py: fx fy cx cy w h near far and the 16 floats of a pose on the command line, the 16 floats of the
// MVP on stdout as their bit patterns.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ifx_host.hpp"

int main(int argc, char** argv)
{
    if (argc != 1 + 8 + 16) return 2;
    double a[8];
    for (int k = 0; k < 8; k++) a[k] = std::strtod(argv[1 + k], nullptr);
    Matrix4f pose;
    for (int k = 0; k < 16; k++) pose.m[k] = std::strtof(argv[9 + k], nullptr);
    const Matrix4f m = viewerMvp(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], pose);
    for (int k = 0; k < 16; k++) {
        uint32_t u;
        std::memcpy(&u, &m.m[k], 4);
        std::printf("%08x\n", u);
    }
    return 0;
}
