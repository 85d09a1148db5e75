"""The BBFRAME layer in plain Python / NumPy, written from the format's description (include/dvbs2hip.h, "BBFRAME layer") and not from the kernels: byte by byte, frame by
frame, in stream order.  tests/test_bbframe_cpu.py pins it to known answers; tests/test_bbframe_gpu.py holds the library to it bit for bit.

  crc8(data, reg=0)                       g(x) = x^8 + x^7 + x^6 + x^4 + x^2 + 1, bit by bit
  build(stream, K_bch, state, params)     -> (bits int32[F, K_bch], state), F = ceil(len(stream) / D)
  parse(bits, valid, state, params)       -> (packets uint8[n, UPLB], status uint8[n], hdr int32[F, 8], counters [5], state)
States are plain dicts (tx_state(), rx_state()); neither function changes the one it is given."""
import numpy as np

DEFAULTS = dict(matype1=0xF2, matype2=0, upl=1504, sync=0x47, mark_tei=False)


def crc8(data, reg=0):
    for b in bytes(data):
        reg ^= b
        for _ in range(8):
            reg = ((reg << 1) ^ 0xD5) & 0xFF if reg & 0x80 else reg << 1
    return reg


_STEP = np.array([crc8([b]) for b in range(256)], np.uint8)      # the register after one byte, from register 0: crc8(m + [b]) = _STEP[crc8(m) ^ b]


def _crc8_fast(data, reg=0):
    for b in bytes(data):
        reg = int(_STEP[reg ^ b])
    return reg


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def tx_state():
    return dict(pos=0, run=0, last=0)


def rx_state():
    return dict(buf=b"", have=False, counters=[0, 0, 0, 0, 0])


def header(p, dfl, syncd):
    h = bytes([p["matype1"], p["matype2"], p["upl"] >> 8, p["upl"] & 255, dfl >> 8, dfl & 255, p["sync"], syncd >> 8, syncd & 255])
    return h + bytes([crc8(h)])


def build(stream, K_bch, state, p=DEFAULTS):
    stream = bytes(np.asarray(stream, np.uint8).tobytes())
    uplb, D = p["upl"] // 8, (K_bch - 80) // 8
    pos, run, last = state["pos"], state["run"], state["last"]
    F = -(-len(stream) // D)
    frames = np.zeros((F, K_bch // 8), np.uint8)
    for f in range(F):
        chunk = stream[f * D:(f + 1) * D]
        d = (uplb - pos) % uplb
        out = bytearray()
        for b in chunk:
            if pos == 0:
                out.append(last)                       # the CRC-8 of the packet before takes the sync byte's place
                run = 0
            else:
                out.append(b)
                run = int(_STEP[run ^ b])
            pos += 1
            if pos == uplb:
                pos, last = 0, run
        dfl = 8 * len(chunk)
        frame = header(p, dfl, 8 * d if 8 * d < dfl else 65535) + bytes(out)
        frames[f, :len(frame)] = np.frombuffer(frame, np.uint8)
    return np.unpackbits(frames, axis=1).astype(np.int32), dict(pos=pos, run=run, last=last)


def parse(bits, valid, state, p=DEFAULTS):
    bits = np.asarray(bits)
    K_bch = bits.shape[-1]
    frames = np.packbits((bits.reshape(-1, K_bch) != 0).astype(np.uint8), axis=1)
    F, uplb = len(frames), p["upl"] // 8
    buf, have = state["buf"], state["have"]
    taken, dropped, ok, bad, disc = state["counters"]
    packets, status, hdr = [], [], np.zeros((F, 8), np.int32)

    def emit(pkt, slot):
        s = int(_crc8_fast(pkt[1:]) != slot)
        pkt = bytearray(pkt)
        pkt[0] = p["sync"]
        if s and p["mark_tei"] and p["upl"] == 1504:
            pkt[1] |= 0x80
        packets.append(bytes(pkt))
        status.append(s)

    for f in range(F):
        fr = bytes(frames[f])
        h = fr[:10]
        upl, dfl, sync, syncd, comp = h[2] << 8 | h[3], h[4] << 8 | h[5], h[6], h[7] << 8 | h[8], crc8(h[:9])
        if valid is not None and valid[f] == 0:
            st = 3
        elif comp != h[9]:
            st = 1
        elif upl != p["upl"] or sync != p["sync"] or dfl > K_bch - 80 or dfl % 8 or (syncd != 65535 and (syncd % 8 or syncd >= dfl)):
            st = 2
        else:
            st = 0
        hdr[f] = [st, h[0] << 8 | h[1], upl, dfl, sync, syncd, h[9], comp]
        if st != 0:
            dropped += 1
            disc += len(buf); buf, have = b"", False
            continue
        taken += 1
        df = fr[10:10 + dfl // 8]
        if syncd == 65535:
            disc += len(buf) + len(df); buf, have = b"", False
            continue
        s = syncd // 8
        if have and len(buf) + s == uplb:
            emit(buf + df[:s], df[s])
        else:
            disc += len(buf) + s
        start = s
        while start + uplb < len(df):
            emit(df[start:start + uplb], df[start + uplb])
            start += uplb
        buf, have = df[start:], True
    ok += status.count(0); bad += status.count(1)
    pk = np.frombuffer(b"".join(packets), np.uint8).reshape(-1, uplb) if packets else np.zeros((0, uplb), np.uint8)
    return pk, np.array(status, np.uint8), hdr, [taken, dropped, ok, bad, disc], dict(buf=buf, have=have, counters=[taken, dropped, ok, bad, disc])


def ts_stream(n_packets, seed=0, upl=1504, sync=0x47):
    """n_packets random packets with their sync byte -> uint8[n_packets * UPLB]"""
    x = np.random.default_rng(seed).integers(0, 256, (n_packets, upl // 8), dtype=np.uint8)
    x[:, 0] = sync
    return x.ravel()
