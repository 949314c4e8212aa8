"""The TCP checksum arithmetic the CPU models share: the 16-bit helpers and
the two pseudo-header sums, the RFC's and the reference's."""
import struct


def _bswap16(x: int) -> int:
    return ((x & 0xFF) << 8) | ((x >> 8) & 0xFF)


def _fold(x: int) -> int:
    while x >> 16:
        x = (x & 0xFFFF) + (x >> 16)
    return x


def pseudo_rfc(saddr: bytes, daddr: bytes, l4len: int) -> int:
    """RFC 1071 pseudo header over the header's words as stored, carries kept."""
    s = sum(struct.unpack("<4H", saddr + daddr))
    return s + _bswap16(6) + _bswap16(l4len)


def lost_carry_seed(saddr: bytes, daddr: bytes, l4len: int) -> int:
    """tcp_udp_checksum's start value (src/tcp.c:92-95): the addresses as
    stored, as u32 words, added in a u32; the carry out of bit 31 is lost."""
    return (int.from_bytes(saddr, "little") + int.from_bytes(daddr, "little") + _bswap16(6)
            + _bswap16(l4len)) & 0xFFFFFFFF
