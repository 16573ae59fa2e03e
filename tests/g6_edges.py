"""The edge list of tests/native/check_g6text.cpp (its `edges` mode prints the same
bit patterns; tests/test_g6_text.py holds the two lists together), and the text
`ostream << float` gives for a binary32 bit pattern, from Python's own '%g'."""
import numpy as np

EDGE_BITS = [
    # 0, -0, inf, -inf, nan, -nan, NaNs with payloads
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF,
    # one output of every length from 1 to 12
    0x3F800000, 0xBF800000, 0x3F000000, 0x3FA00000, 0xBFA00000, 0x49742400, 0x47F12000, 0x505F8476, 0xD05F8476,
    0x2F09705F, 0x5037E15D, 0x5037F470, 0x5037F6BA, 0xD037F6BA, 0x390173F8, 0xB90173F8, 0x80800000,
    # 1e-5 | 1e-4 with the round-up carry 9.999995e-5
    0x3727C5AC, 0x38D1B70A, 0x38D1B710, 0x38D1B717, 0x38D1B717, 0x38D1B7A1,
    # 999999 | 1e+06 with the half-even ties at 999999.5, 999998.5, 999997.5
    0x497423F0, 0x497423F8, 0x497423F7, 0x497423E8, 0x497423D8, 0x49742400, 0x49742410, 0x47C35000, 0x47C34FFA,
    # the ends of the range, two-digit exponents of both signs
    0x00000001, 0x00000002, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x501502F9, 0x2EDBE6FF, 0x7E967699, 0x006CE3EE,
    0x00000001,
    # plain values, trailing zeros, a bare point
    0x3DCCCCCD, 0x3A83126F, 0x42C80000, 0x47C35000, 0x4640E666, 0x47F1205A, 0x3FC00000, 0x3E99999A, 0x4B800000,
    0x40490FDB, 0xB48637BD,
]


def g_text(bits: int) -> str:
    """snprintf("%g") of the binary32 with these bits (glibc's spelling of inf and nan)."""
    a = bits & 0x7FFFFFFF
    sign = "-" if bits >> 31 else ""
    if a == 0x7F800000:
        return sign + "inf"
    if a > 0x7F800000:
        return sign + "nan"
    return "%g" % float(np.array([bits], np.uint32).view(np.float32)[0])


def edge_values() -> np.ndarray:
    return np.array(EDGE_BITS, np.uint32).view(np.float32)
