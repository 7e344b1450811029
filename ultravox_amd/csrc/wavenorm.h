// Constants of the raw-waveform normaliser (wavenorm.hip; the definition is uvx_wave_norm's comment in include/uvx.h).
#pragma once
#include <stdint.h>

namespace uvx {
namespace wavenorm {

constexpr int THREADS = 256;       // both kernels
constexpr int CHUNK = 16384;       // samples of one row, counted from the row's own start, that one block reduces to one (S1, S2) pair
constexpr int TILE = 4096;         // outputs of one row that one block of the second launch writes
constexpr double EPS = 1e-7;       // zero_mean_unit_var_norm's epsilon

}  // namespace wavenorm
}  // namespace uvx
