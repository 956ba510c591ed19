// What the tests/emu and tests/sim programs share for the contract builds and the saturated cases (test infrastructure).
// Include after bb_field.hpp (any header of toyni_amd/csrc).
#pragma once

// the contract builds (tests/emu/field_contracts.hpp, tests/test_field_contracts.py) name the case a violation belongs to;
// a plain build names nothing
#ifndef TOYNI_CONTRACT_TAG
#define TOYNI_CONTRACT_TAG(...) ((void)0)
#endif

// Saturated operands: 1069547521 is the plain value whose Montgomery form is p - 1, so with it as every caller-supplied constant and
// p - 1 as every data word, each product a kernel forms between a data word and a constant is (p - 1)^2
constexpr uint32_t SAT_X = 1069547521u;
static_assert((uint32_t)((((uint64_t)SAT_X) << 32) % toyni::BB_P) == toyni::BB_P - 1u, "Montgomery form p - 1");
