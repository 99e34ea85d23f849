// host_common.h -- what every host-side unit of the library needs: HIP_CHECK, logging, the calling thread's last-error string
// and the try/catch pair that turns an exception into a C-ABI return value.
#pragma once
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "../../include/tcnn_hip.h"
#include "tcnn_device.h"

namespace tcnn_hip {

#define HIP_CHECK(x)                                                                                        \
	do {                                                                                                    \
		hipError_t e_ = (x);                                                                                \
		if (e_ != hipSuccess) throw std::runtime_error(std::string(#x " failed: ") + hipGetErrorString(e_)); \
	} while (0)

// logging (common_host.h:46-69) and the calling thread's error string behind tcnn_last_error(); both defined in api_switches.hip
void log_message(int severity, const std::string& msg);
void set_last_error(const std::string& msg);

// this build's 16-bit type (tcnn_device.h): fp16, or bfloat16 when compiled with -DTCNN_BF16
constexpr int NATIVE_PRECISION = HALF_IS_BF16 ? TCNN_PRECISION_BF16 : TCNN_PRECISION_FP16;

// body of a C-ABI function that reports through its return value: an exception becomes the last error, a log line and TCNN_ERROR
#define TCNN_API_BEGIN try {
#define TCNN_API_END                                       \
	}                                                      \
	catch (const std::exception& ex) {                     \
		tcnn_hip::set_last_error(ex.what());               \
		tcnn_hip::log_message(TCNN_LOG_ERROR, ex.what());  \
		return TCNN_ERROR;                                 \
	}                                                      \
	return TCNN_OK;

}  // namespace tcnn_hip
