// hip_check.hpp -- HIP_CHECK: a failed HIP runtime call is logged and thrown as a FatalError carrying
// the HIP error string.
#pragma once

#include "common.hpp"

#include <hip/hip_runtime_api.h>

#include <string>

#define HIP_CHECK(expr)                                                         \
    do {                                                                        \
        hipError_t e_ = (expr);                                                 \
        if (e_ != hipSuccess) {                                                 \
            std::string m_ = std::string("HIP failure: ") + #expr + ": " +      \
                             hipGetErrorString(e_);                             \
            log_msg(LOG_ERR, "%s\n", m_.c_str());                               \
            throw FatalError(m_);                                               \
        }                                                                       \
    } while (0)
