// Stand-alone host program of the hinge builder (csrc/bending.hpp; no HIP, plain g++). Reads
// meshes from argv[1], each "<name> <n verts> <n tris> <k_bend> <flat_rest>" followed by the
// vertices (3 numbers each; nan / inf accepted) and the triangles (3 indices each), and prints per mesh
//   mesh <name> <n hinges>
//   h <x0> <x1> <x2> <x3> <K0> <K1> <K2> <K3> <kappa> <r>        (one line per hinge, %.17g)
// or, for a refused mesh,
//   error <name> <code> <message>
// tests/test_bending.py compares the lines with the numpy restatement (tests/bending_cases.py).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "bending.hpp"

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: bending meshes.txt\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::printf("cannot open %s\n", argv[1]); return 2; }
    std::string name, tok;
    int n_meshes = 0;
    while (in >> name) {
        int nv = 0, nf = 0, flat = 1;
        std::string kb;
        if (!(in >> nv >> nf >> kb >> flat)) { std::printf("bad header of %s\n", name.c_str()); return 2; }
        const double k_bend = std::strtod(kb.c_str(), nullptr);
        std::vector<double> V(3 * (size_t)nv);
        std::vector<int> F(3 * (size_t)nf);
        for (auto& c : V) { if (!(in >> tok)) return 2; c = std::strtod(tok.c_str(), nullptr); }
        for (auto& i : F) if (!(in >> i)) return 2;
        try {
            const aa::HingeSet H = aa::build_hinges(V.data(), nv, F.data(), nf, k_bend, flat != 0);
            std::printf("mesh %s %d\n", name.c_str(), H.count());
            for (int e = 0; e < H.count(); ++e)
                std::printf("h %d %d %d %d %.17g %.17g %.17g %.17g %.17g %.17g\n", H.idx[4 * e], H.idx[4 * e + 1], H.idx[4 * e + 2],
                            H.idx[4 * e + 3], H.K[4 * e], H.K[4 * e + 1], H.K[4 * e + 2], H.K[4 * e + 3], H.kappa[e], H.r[e]);
        } catch (const aa::Error& err) {
            std::printf("error %s %d %s\n", name.c_str(), err.code, err.what());
        }
        ++n_meshes;
    }
    std::printf("ok %d meshes\n", n_meshes);
    return 0;
}
