// Status codes and the exception every layer throws (mapped to the C ABI's codes in capi.cpp).
// No HIP: the host-only headers (bvh_build.hpp, mesh_obstacle.hpp) build with a plain compiler.
#pragma once
#include <stdexcept>
#include <string>

namespace aa {

enum Status { OK = 0, ERR_ARG = -1, ERR_STATE = -2, ERR_DEVICE = -3, ERR_NUMERIC = -4 };

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

}  // namespace aa
