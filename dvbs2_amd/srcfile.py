"""The reference's payload sources and its sink as files (DVBS2.cpp:359-389; the modules themselves live in StreamPU, absent from /root/reference):

  Source_user         conf/src/K_14232.src, K_9552.src: text, `n_frames`, `K`, then n_frames * K bits; the source cycles through the frames (DVBS2.cpp:367)
  Source_user_binary  `--src-type USER_BIN --src-path video.ts` (README.md:203): any file, eight payload bits per byte, the file's first bit in the least significant
                      bit of its first byte [UPSTREAM-RECALL: spu::tools::Bit_packer's default order]; at the end of the file it starts over (`--src-no-loop`: the last
                      frame is zero-padded and the source is done) (DVBS2.cpp:369)
  Source_AZCW         all-zero payloads (DVBS2.cpp:371)
  Sink_user_binary    `--snk-path out.ts` (README.md:210): the decoded payload packed the same way, frame after frame (DVBS2.cpp:385)

A file sent with USER_BIN and received into the sink is the file again, byte for byte, whatever the bit order -- both ends use the same one.

An extension beside them: SourceTS / SinkTS (`--src-type TS`, `--snk-type TS`), a transport stream as the packet stream of the BBFRAME layer (Dvbs2Hip.bbframe_build /
bbframe_parse / rx_bb_up): the frames on air are DVB-S2 BBFRAMEs, and the sink gets whole packets of the frames whose BBHEADER checks."""
from __future__ import annotations

import numpy as np


def load_src(path: str, K: int | None = None) -> np.ndarray:
    """-> int32 [n_frames, K]"""
    tok = open(path).read().split()
    if len(tok) < 2:
        raise ValueError("'%s' is not a source pattern file" % path)
    n, k = int(tok[0]), int(tok[1])
    if K is not None and k != K:
        raise ValueError("'%s' holds frames of %d bits, the MODCOD needs %d" % (path, k, K))
    bits = np.array(tok[2:2 + n * k], dtype=np.int32)
    if bits.size != n * k or ((bits != 0) & (bits != 1)).any():
        raise ValueError("'%s' is truncated or holds something else than bits" % path)
    return bits.reshape(n, k)


def save_src(path: str, bits) -> None:
    b = np.atleast_2d(np.asarray(bits, dtype=np.int32))
    with open(path, "w") as f:
        f.write("%d\n%d\n" % b.shape)
        for row in b:
            f.write(" ".join(map(str, row.tolist())) + " \n")


class SourceUser:
    """generate(F) -> the next F frames of the pattern, cyclically (auto_reset = true)"""

    def __init__(self, path: str, K: int):
        self.frames = load_src(path, K)
        self.pos = 0

    def generate(self, F: int) -> np.ndarray:
        idx = (self.pos + np.arange(F)) % self.frames.shape[0]
        self.pos = int((self.pos + F) % self.frames.shape[0])
        return self.frames[idx]


class SourceDone(RuntimeError):
    """the source has no more frames (a USER_BIN file without looping has been sent)"""


class SourceUserBinary:
    """generate(F) -> the next F frames of K bits from a binary file, int32 [F, K]"""

    def __init__(self, path: str, K: int, auto_reset: bool = True):
        if K % 8:
            raise ValueError("K = %d is not a whole number of bytes" % K)
        import os
        if os.path.getsize(path) == 0:
            raise ValueError("'%s' is empty" % path)
        self.data = np.memmap(path, dtype=np.uint8, mode="r")          # (a transport stream of gigabytes stays on disk)
        self.K, self.pos, self.auto_reset, self.done = K, 0, auto_reset, False

    def generate(self, F: int) -> np.ndarray:
        if self.done:
            raise SourceDone("the whole file has been sent")
        nb = F * self.K // 8
        if self.auto_reset:
            idx = (self.pos + np.arange(nb)) % self.data.size
            chunk = np.asarray(self.data[idx])
            self.pos = int((self.pos + nb) % self.data.size)
        else:
            chunk = np.zeros(nb, np.uint8)
            left = self.data[self.pos:self.pos + nb]
            chunk[:left.size] = left
            self.pos += left.size
            if self.pos >= self.data.size:
                self.done = True
        return np.unpackbits(chunk, bitorder="little").astype(np.int32).reshape(F, self.K)

    def frames_left(self) -> int | None:
        """whole or partial frames still to come (None: a looping source never ends)"""
        return None if self.auto_reset else -(-(self.data.size - self.pos) * 8 // self.K)


TS_PACKET, TS_SYNC = 188, 0x47
TS_NULL = np.concatenate([np.array([TS_SYNC, 0x1F, 0xFF, 0x10], np.uint8), np.full(TS_PACKET - 4, 0xFF, np.uint8)])       # PID 0x1FFF, payload only


class SourceTS:
    """An MPEG transport stream as the BBFRAME layer's packet stream (`--src-type TS`): generate(F) -> (the next bytes of the stream, the frames they fill), what
    Dvbs2Hip.bbframe_build takes; D = (K_bch - 80) / 8 bytes go into a full frame.  The file has to be whole packets of 188 bytes that start with 0x47.  It loops over the
    file (packets keep straddling frames across the wrap); auto_reset = False sends it once, followed by one null packet that gives the file's last packet the CRC slot
    behind it -- the last frame is then short -- and then by one call of no frames at all (the transmitter pads it), which pushes the last frames through a receiver's
    delays."""

    def __init__(self, path: str, D: int, auto_reset: bool = True):
        import os
        size = os.path.getsize(path)
        if size == 0:
            raise ValueError("'%s' is empty" % path)
        self.data = np.memmap(path, dtype=np.uint8, mode="r")
        if size % TS_PACKET:
            raise ValueError("'%s' is not a transport stream: %d bytes are not whole packets of 188 (offset %d)" % (path, size, size - size % TS_PACKET))
        bad = np.flatnonzero(np.asarray(self.data[::TS_PACKET]) != TS_SYNC)
        if bad.size:
            raise ValueError("'%s' is not a transport stream: no sync byte 0x47 at offset %d" % (path, int(bad[0]) * TS_PACKET))
        self.D, self.pos, self.auto_reset, self.done, self.flushed = int(D), 0, auto_reset, False, False
        self.size = size if auto_reset else size + TS_PACKET

    def generate(self, F: int):
        nb = F * self.D
        if self.auto_reset:
            idx = (self.pos + np.arange(nb)) % self.size
            self.pos = int((self.pos + nb) % self.size)
            return np.asarray(self.data[idx]), F
        if self.done:
            if self.flushed:
                raise SourceDone("the whole file has been sent")
            self.flushed = True
            return np.zeros(0, np.uint8), 0
        end = min(self.pos + nb, self.size)
        chunk = np.concatenate([np.asarray(self.data[self.pos:min(end, self.data.size)]), TS_NULL[max(self.pos, self.data.size) - self.data.size:max(end, self.data.size) - self.data.size]])
        self.pos = end
        self.done = end >= self.size
        return chunk, -(-chunk.size // self.D)


class SinkTS:
    """send(packets[n, 188]) appends the packets the BBFRAME parser emitted (`--snk-type TS`)"""

    def __init__(self, path: str):
        self.f = open(path, "wb")

    def send(self, packets) -> None:
        self.f.write(np.ascontiguousarray(packets, dtype=np.uint8).tobytes())
        self.f.flush()

    def close(self) -> None:
        self.f.close()


class SourceAZCW:
    def __init__(self, K: int):
        self.K = K

    def generate(self, F: int) -> np.ndarray:
        return np.zeros((F, self.K), np.int32)


class SinkUserBinary:
    """send(bits[F, K]) appends the frames to the file, eight bits per byte"""

    def __init__(self, path: str, K: int):
        if K % 8:
            raise ValueError("K = %d is not a whole number of bytes" % K)
        self.K, self.f = K, open(path, "wb")

    def send(self, bits) -> None:
        b = np.ascontiguousarray(bits).reshape(-1, self.K)
        self.f.write(np.packbits((b != 0).astype(np.uint8), axis=1, bitorder="little").tobytes())
        self.f.flush()                                               # (the sink may be a FIFO with a player behind it: README.md:206-217 of the reference)

    def close(self) -> None:
        self.f.close()
