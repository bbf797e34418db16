// sam_host.hpp - what the host side of the SAM front end shares: strtod for the floats the fast path leaves alone, the header's dictionary (sam_host.cpp).
#pragma once
#include "sam_core.hpp"
#include <string>
#include <vector>

bool sam_host_strtod(const uint8_t* s, uint32_t n, float* out);
// the @SQ dictionary (and @HD SO) of a header text; SVX_E_ARG: an @SQ line without SN or LN
int sam_header_parse(const char* text, size_t n, std::vector<std::string>* names, std::vector<int32_t>* lengths, std::string* sort_order);
