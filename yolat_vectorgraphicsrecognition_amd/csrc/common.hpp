// common.hpp — umbrella over the shared headers of libyolat_hip.so, for code outside csrc/ (tools/exp/*.hip).  No file of
// csrc/ includes it: each .hip includes the headers it uses (DESIGN.md "File layout").
#pragma once
#include "base.hpp"
#include "operands.hpp"
#include "epilogue.hpp"
#include "gemm_nt.hpp"
#include "gemm_nt_two.hpp"
#include "internal.hpp"
#include "gemm_sk.hpp"
#include "gemm_tn.hpp"
