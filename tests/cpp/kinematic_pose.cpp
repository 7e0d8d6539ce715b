// Pose validation of the kinematic mesh obstacle (csrc/mesh_obstacle.hpp), no GPU:
//   * validate_mesh_pose accepts the poses given in argv[1] (tests/kinematic_cases.py's, one per
//     line: R row-major, then t) and the identity;
//   * it refuses, with ERR_ARG and a message naming the cause, each of them mirrored (det R < 0),
//     scaled (1.001 R), with a NaN in R and with an infinite t;
//   * apply_mesh_pose writes R, t and the flag into a table row, and a null pose resets the row
//     to unposed with the identity.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <limits>
#include <string>
#include <vector>

#include "mesh_obstacle.hpp"

namespace {
int fails = 0;
void expect(bool ok, const std::string& what) {
    if (!ok) { std::printf("FAIL %s\n", what.c_str()); ++fails; }
}
void refused(const std::vector<double>& p, const std::string& needle, const std::string& what) {
    try {
        aa::validate_mesh_pose(p.data(), "test: ");
        expect(false, what + ": accepted");
    } catch (const aa::Error& e) {
        expect(e.code == aa::ERR_ARG, what + ": not ERR_ARG");
        expect(std::string(e.what()).find(needle) != std::string::npos, what + ": message '" + e.what() + "' lacks '" + needle + "'");
    }
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    std::vector<std::vector<double>> poses;
    for (;;) {
        std::vector<double> p(12);
        bool ok = true;
        for (double& v : p) ok = ok && (in >> v);
        if (!ok) break;
        poses.push_back(p);
    }
    expect(!poses.empty(), "no poses read");
    const std::vector<double> id = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    try { aa::validate_mesh_pose(id.data(), "test: "); } catch (const aa::Error& e) { expect(false, std::string("identity refused: ") + e.what()); }
    for (size_t k = 0; k < poses.size(); ++k) {
        const std::vector<double>& p = poses[k];
        const std::string tag = "pose " + std::to_string(k);
        try { aa::validate_mesh_pose(p.data(), "test: "); } catch (const aa::Error& e) { expect(false, tag + " refused: " + e.what()); }
        std::vector<double> q = p;
        for (int i = 0; i < 3; ++i) q[6 + i] = -q[6 + i];   // last row negated: a reflection
        refused(q, "reflection", tag + " mirrored");
        q = p;
        for (int i = 0; i < 9; ++i) q[i] *= 1.001;
        refused(q, "not orthonormal", tag + " scaled");
        q = p;
        q[4] = std::nan("");
        refused(q, "not finite", tag + " with NaN");
        q = p;
        q[10] = std::numeric_limits<double>::infinity();
        refused(q, "not finite", tag + " with an infinite t");

        aa::MeshObsDev d{};
        aa::apply_mesh_pose(d, p.data());
        bool same = d.posed == 1;
        for (int i = 0; i < 9; ++i) same = same && d.R[i] == p[i];
        for (int i = 0; i < 3; ++i) same = same && d.t[i] == p[9 + i];
        expect(same, tag + ": row not written");
        aa::apply_mesh_pose(d, nullptr);
        same = d.posed == 0;
        for (int i = 0; i < 9; ++i) same = same && d.R[i] == id[i];
        for (int i = 0; i < 3; ++i) same = same && d.t[i] == 0.0;
        expect(same, tag + ": row not reset");
    }
    if (fails) return 1;
    std::printf("ok %zu poses\n", poses.size());
    return 0;
}
