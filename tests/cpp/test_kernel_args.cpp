// Host and device side of every kernel argument block (heyoka_amd/csrc/kernel_args.hpp), compared by the compiler: for each
// block of HY_KARGS_BLOCKS one empty kernel over the device text of the block, all of them compiled in one module for
// gfx950 (no GPU is needed); the code object goes to the file named on the command line, and one line "<device struct>
// <sizeof of the host struct>" per block to the standard output. tests/test_kernel_args.py reads the size of the argument
// segment of every kernel from the code object and compares.
#include <cstddef>
#include <cstdio>
#include <string>
#include <vector>

#include "heyoka_amd.h"
#include "kernel_args.hpp"

using namespace heyoka_amd;
using namespace heyoka_amd::detail;

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: test_kernel_args CODE_OBJECT_FILE\n");
        return 2;
    }
    std::string src = "typedef unsigned long long u64;\ntypedef long long i64;\n";
#define HY_X(host, dev) src += host##_text() + "extern \"C\" __global__ void k_" #dev "(const " #dev " a) {}\n";
    HY_KARGS_BLOCKS(HY_X)
#undef HY_X
    std::size_t n = 0;
    if (hy_hiprtc_compile(src.c_str(), nullptr, &n) != 0) {
        std::fprintf(stderr, "%s\n%s", hy_last_error(), src.c_str());
        return 1;
    }
    std::vector<char> co(n);
    if (hy_hiprtc_compile(src.c_str(), co.data(), &n) != 0) {
        std::fprintf(stderr, "%s\n", hy_last_error());
        return 1;
    }
    std::FILE *f = std::fopen(argv[1], "wb");
    if (f == nullptr || std::fwrite(co.data(), 1, n, f) != n || std::fclose(f) != 0) {
        std::fprintf(stderr, "cannot write %s\n", argv[1]);
        return 1;
    }
#define HY_X(host, dev) std::printf(#dev " %zu\n", sizeof(host));
    HY_KARGS_BLOCKS(HY_X)
#undef HY_X
    return 0;
}
