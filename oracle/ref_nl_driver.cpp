// Stand-alone driver around the reference's own NL/ sources (qx_tree_filter, qx_mst_kruskals_image,
// ctmf), built by oracle/ref_nl.mk from adapted copies in oracle/_ref/src/.  TEST INFRASTRUCTURE ONLY:
// it gives the tests an answer that is not a restatement.
//
//   ref_nl_driver IN OUT
//
// IN : int32 H, W, P, mode; float64 sigma; H*W*3 bytes (BGR, row-major); H*W*P float32 ([pixel][plane]).
// OUT: mode 0 "median": H*W*3 bytes, ctmf called as qx_mst_kruskals_image::mst() calls it.
//      mode 1 "tree"  : after init(h, w, 3, 4) and mst(img), the public getters, n = H*W:
//                       int32 parent[n], nr_child[n], children[n][3] (-1 past nr_child), uint8 weight[n],
//                       int32 node_id[n] (the breadth-first order), rank[n].
//      mode 2 "filter": what NLCCA::aggreCV does: floats widened to double, qx_tree_filter::init(h, w, 3,
//                       sigma, 4), build_tree(img), filter(cost, temp, P), narrowed back with (float).
// Exit status 0 on success, 2 on a malformed call; ctmf's own assert() aborts on sizes it cannot do.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "qx_basic.h"
#include "qx_tree_filter.h"

namespace {

bool read_all(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
bool write_all(FILE *f, const void *p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }

int fail(const char *what) {
    fprintf(stderr, "ref_nl_driver: %s\n", what);
    return 2;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) return fail("usage: ref_nl_driver IN OUT");
    FILE *in = fopen(argv[1], "rb");
    if (!in) return fail("cannot open the input file");
    int32_t hdr[4];
    double sigma;
    if (!read_all(in, hdr, sizeof hdr) || !read_all(in, &sigma, sizeof sigma)) return fail("short header");
    const int h = hdr[0], w = hdr[1], planes = hdr[2], mode = hdr[3];
    if (h < 1 || w < 1 || planes < 0 || mode < 0 || mode > 2) return fail("bad header");
    const size_t n = (size_t)h * (size_t)w;
    std::vector<unsigned char> img(n * 3);
    std::vector<float> vol(n * (size_t)planes);
    if (!read_all(in, img.data(), img.size()) || !read_all(in, vol.data(), vol.size() * sizeof(float)))
        return fail("short payload");
    fclose(in);

    FILE *out = fopen(argv[2], "wb");
    if (!out) return fail("cannot open the output file");
    bool ok = true;
    if (mode == 0) {
        std::vector<unsigned char> med(n * 3);
        ctmf(img.data(), med.data(), w, h, w * 3, w * 3, 1, 3, (unsigned long)(h * w * 3));
        ok = write_all(out, med.data(), med.size());
    } else if (mode == 1) {
        qx_mst_kruskals_image mst;
        mst.init(h, w, 3, 4);
        mst.mst(img.data());
        std::vector<int32_t> children(n * 3, -1);
        const int *nr_child = mst.get_nr_child();
        int **ch = mst.get_children();
        for (size_t i = 0; i < n; i++)
            for (int j = 0; j < nr_child[i] && j < 3; j++) children[i * 3 + j] = ch[i][j];
        ok = write_all(out, mst.get_parent(), n * sizeof(int)) && write_all(out, nr_child, n * sizeof(int)) &&
             write_all(out, children.data(), children.size() * sizeof(int32_t)) &&
             write_all(out, mst.get_weight(), n) && write_all(out, mst.get_node_id(), n * sizeof(int)) &&
             write_all(out, mst.get_rank(), n * sizeof(int));
    } else {
        std::vector<double> cost(vol.size()), temp(vol.size());
        for (size_t i = 0; i < vol.size(); i++) cost[i] = (double)vol[i];
        qx_tree_filter tf;
        tf.init(h, w, 3, sigma, 4);
        tf.build_tree(img.data());
        tf.filter(cost.data(), temp.data(), planes);
        for (size_t i = 0; i < vol.size(); i++) vol[i] = (float)cost[i];
        ok = write_all(out, vol.data(), vol.size() * sizeof(float));
    }
    if (fclose(out) != 0 || !ok) return fail("cannot write the output file");
    return 0;
}
