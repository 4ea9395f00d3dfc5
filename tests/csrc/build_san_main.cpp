// Stand-alone program for a sanitizer build of lpc_build.hpp and the model walk
// (tests/test_build_host.py compiles it with -fsanitize=address,undefined and runs
// it as a child process).  argv[1]: a file of cases written by the test,
//   int32 ncases, then per case:
//   int32 M, int32 n, int32 half, float max_ray_len, double dcap, double scene_scale,
//   float v0[M][4], v1[M][4], v2[M][4], int32 mesh_id[M], float origin[n][4], dir[n][4]
// Per case: the records with 1 and 5 threads must be the same bytes, a build with
// a stack too small for the hierarchy must be refused, and the model walk must
// equal brute force.  Exit status 0 when all hold.
#include <cstdio>

#include "build_model.hpp"

using namespace bm;

template <class T>
static bool read_vec(FILE *f, std::vector<T> &v, size_t count)
{
    v.resize(count);
    return count == 0 || fread(v.data(), sizeof(T), count, f) == count;
}

template <class T>
static bool same_bytes(const std::vector<T> &a, const std::vector<T> &b)
{
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t ncases = 0;
    if (fread(&ncases, 4, 1, f) != 1) return 2;
    int bad = 0;
    for (int32_t c = 0; c < ncases; ++c) {
        int32_t M, n, half;
        float max_ray_len;
        double dcap, scale;
        if (fread(&M, 4, 1, f) != 1 || fread(&n, 4, 1, f) != 1 || fread(&half, 4, 1, f) != 1 ||
            fread(&max_ray_len, 4, 1, f) != 1 || fread(&dcap, 8, 1, f) != 1 || fread(&scale, 8, 1, f) != 1)
            return 2;
        std::vector<float> v0, v1, v2, o4, d4;
        std::vector<int32_t> mesh_id;
        if (!read_vec(f, v0, 4 * (size_t)M) || !read_vec(f, v1, 4 * (size_t)M) || !read_vec(f, v2, 4 * (size_t)M) ||
            !read_vec(f, mesh_id, (size_t)M) || !read_vec(f, o4, 4 * (size_t)n) || !read_vec(f, d4, 4 * (size_t)n))
            return 2;
        Built A, B5, deep;
        build(A, M, v0.data(), v1.data(), v2.data(), mesh_id.data(), dcap, scale, 1.0, 64, 1);
        build(B5, M, v0.data(), v1.data(), v2.data(), mesh_id.data(), dcap, scale, 1.0, 64, 5);
        if (!A.err.empty() || !B5.err.empty()) { fprintf(stderr, "case %d: build refused: %s\n", c, A.err.c_str()); ++bad; continue; }
        bool same = same_bytes(A.out.nodes, B5.out.nodes) && same_bytes(A.out.node_self, B5.out.node_self) &&
                    same_bytes(A.out.slivers, B5.out.slivers) && same_bytes(A.out.xorder, B5.out.xorder) &&
                    same_bytes(A.out.run_slo, B5.out.run_slo) && same_bytes(A.out.run_shi, B5.out.run_shi) &&
                    A.out.run_levels == B5.out.run_levels;
        if (!same) { fprintf(stderr, "case %d: records differ between 1 and 5 threads\n", c); ++bad; }
        size_t levels = 0;
        for (const auto &l : A.out.run_levels) levels = std::max(levels, l.size() / 2);
        if (levels) {
            build(deep, M, v0.data(), v1.data(), v2.data(), mesh_id.data(), dcap, scale, 1.0, 7 * (int)levels, 3);
            if (deep.err.empty()) { fprintf(stderr, "case %d: a stack of %d was not refused\n", c, 7 * (int)levels); ++bad; }
        }
        const size_t nr = A.run_lo.size();
        std::vector<float> bt((size_t)n * nr);
        std::vector<int32_t> bi((size_t)n * nr), bc((size_t)n * nr);
        const WalkStats W = model_walk(A, v0.data(), v1.data(), v2.data(), n, o4.data(), d4.data(), max_ray_len, half != 0,
                                       bt.data(), bi.data(), bc.data());
        long long hits = 0;
        for (int32_t x : bc) hits += x > 0;
        printf("case %d: M %d runs %zu nodes %zu slivers %zu rays %d compared %lld mismatches %lld hit slots %lld\n", c, M, nr,
               A.out.nodes.size(), A.out.slivers.size(), n, W.compared, W.mismatches, hits);
        if (W.mismatches) ++bad;
    }
    fclose(f);
    return bad ? 1 : 0;
}
