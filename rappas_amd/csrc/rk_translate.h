// rk_translate.h -- six-frame translation of packed DNA records: the codon table shared by translate_frame_kernel
// (rk_kernels.hip) and its host twin (rk_translate_host.h).  Not part of the C ABI.
#pragma once
#include <stdint.h>

// The standard genetic code (NCBI table 1).  Index = b0 | b1 << 2 | b2 << 4 over the three bases of a codon in reading order, with
// the engine's DNA states A=0 T=1 C=2 G=3 -- the six bits of a forward codon as they lie in a packed record.  Value = residue state
// in the order of AAStates.java:48-197 (R=0 H=1 K=2 D=3 E=4 S=5 T=6 N=7 Q=8 C=9 G=10 P=11 A=12 I=13 L=14 M=15 F=16 W=17 Y=18
// V=19), or RK_CODON_STOP for TAA (index 1), TGA (13) and TAG (49).  Row i below = third base A T C G (16 indices each):
//   K * Q E I L L V T S P A R * R G / N Y H D I F L V T S P A S C R G / N Y H D I F L V T S P A S C R G / K * Q E M L L V T S P A R W R G
#define RK_CODON_STOP 31u
#define RK_CODON_TABLE                                                                                                          \
    { 2, 31, 8, 4, 13, 14, 14, 19, 6, 5, 11, 12, 0, 31, 0, 10, 7, 18, 1, 3, 13, 16, 14, 19, 6, 5, 11, 12, 5, 9, 0, 10,          \
      7, 18, 1, 3, 13, 16, 14, 19, 6, 5, 11, 12, 5, 9, 0, 10, 2, 31, 8, 4, 15, 14, 14, 19, 6, 5, 11, 12, 0, 17, 0, 10 }
