#pragma once
// Width of the phasing vote's banded pair accumulator (np2_regions.hip), for the kernels (np2_kernels.hpp) and for the
// host half of the vote (np2_vote_host.hpp): reads are numbered in start order, so the partners b of read a lie close
// above it, and a pair is held by the band if b - a - 1 < EDGE_BAND.  Host-only: a plain C++ compiler builds it.
#include <cstdint>

namespace np2 {
static constexpr uint32_t EDGE_BAND = 256;
} // namespace np2
