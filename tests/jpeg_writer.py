"""A baseline JPEG writer for the tests: from quantised coefficients to a file, so that a test chooses every bit of the
entropy-coded data (tests/golden/make_jpeg_streams_golden.py builds the stream cases with it).  numpy and struct only; nothing
of the package under test is imported, and ``stats`` -- what the writer emitted -- is counted here, never by a decoder.

    data, stats = write_jpeg(width, height, blocks, quant={0: q}, dc={0: spec}, ac={0: spec})

``blocks``: one entry per component (one for a gray file; Y, Cb, Cr with ``sampling=(hs, vs)``, the luma factors), each a
sequence of the component's blocks in raster order on the MCU-padded grid.  A block is either 64 quantised coefficients in
natural order, or -- the escape -- a list of ``(symbol, value)`` pairs and raw bit strings, emitted as they stand: the first
pair with the component's DC table (``value`` is the DC *difference*; the predictor follows it), the others with its AC
table; ``value`` is coded in ``symbol & 15`` bits (ignored for 0 bits); a ``str`` of ``0`` / ``1`` is written bit for bit.  That
writes what no coefficient array encodes: ZRL in front of EOB, symbols with size 0 and a run below 15, a run past 63.

A Huffman spec is ``(bits[16], values)`` as in a DHT segment; ``huffman_from_lengths`` builds one.
"""
import struct

import numpy as np

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
          62, 63)
EOB, ZRL = 0x00, 0xF0


def huffman_from_lengths(symbols, lengths):
    """The canonical spec ``(bits[16], values)`` in which ``symbols[i]`` has a code of ``lengths[i]`` bits; symbols of one
    length keep their order.  ValueError if a length is outside 1..16, a symbol is repeated or outside 0..255, the lengths
    break Kraft's inequality, or they fill the code space, which would assign the all-ones code (JPEG forbids it)."""
    symbols, lengths = list(symbols), list(lengths)
    if len(symbols) != len(lengths) or not symbols:
        raise ValueError("huffman_from_lengths: %d symbols and %d lengths" % (len(symbols), len(lengths)))
    if len(set(symbols)) != len(symbols) or any(not 0 <= s <= 255 for s in symbols):
        raise ValueError("huffman_from_lengths: symbols must be distinct bytes")
    if any(not 1 <= l <= 16 for l in lengths):
        raise ValueError("huffman_from_lengths: code lengths are 1..16")
    kraft = sum(1 << (16 - l) for l in lengths)
    if kraft > 1 << 16:
        raise ValueError("huffman_from_lengths: the lengths break Kraft's inequality")
    if kraft == 1 << 16:
        raise ValueError("huffman_from_lengths: the lengths fill the code space: the all-ones code would be assigned")
    order = sorted(range(len(symbols)), key=lambda i: lengths[i])  # stable
    return [lengths.count(l) for l in range(1, 17)], [symbols[i] for i in order]


def code_table(spec):
    """``(bits, values)`` -> {symbol: (code, length, is the first code of its length, is the last)}."""
    bits, values = spec
    assert len(bits) == 16 and sum(bits) == len(values) and len(set(values)) == len(values)
    table, code, k = {}, 0, 0
    for l in range(1, 17):
        for j in range(bits[l - 1]):
            table[values[k]] = (code, l, j == 0, j == bits[l - 1] - 1)
            code, k = code + 1, k + 1
        assert code <= 1 << l
        code <<= 1
    return table


def block_grid(width, height, sampling):
    """(MCUs across, MCUs down, [(blocks across, blocks down) per component])."""
    hs, vs = sampling or (1, 1)
    mw, mh = -(-width // (8 * hs)), -(-height // (8 * vs))
    return mw, mh, [(mw * hs, mh * vs)] + ([(mw, mh)] * 2 if sampling else [])


def _size(v):
    return int(abs(int(v))).bit_length()


def block_pairs(coef, pred):
    """64 coefficients in natural order -> the ``(symbol, value)`` list a baseline encoder writes, DC as a difference to
    ``pred``."""
    zz = [int(coef[ZIGZAG[k]]) for k in range(64)]
    diff = zz[0] - pred
    out, run = [(_size(diff), diff)], 0
    last = max([k for k in range(1, 64) if zz[k]] or [0])
    for k in range(1, last + 1):
        if zz[k] == 0:
            run += 1
            continue
        while run > 15:
            out.append((ZRL, 0))
            run -= 16
        out.append((run << 4 | _size(zz[k]), zz[k]))
        run = 0
    if last < 63:
        out.append((EOB, 0))
    return out


class _Segment:
    """The bits of one restart interval and the counts of what went into it."""

    def __init__(self, stats):
        self.bits, self.pos, self.stats = [], 0, stats

    def raw(self, s):
        assert set(s) <= {"0", "1"}
        self.bits.append(s)
        self.pos += len(s)

    def symbol(self, key, table, symbol, value):
        if symbol not in table:
            raise ValueError("jpeg_writer: symbol 0x%02x is not in table %s" % (symbol, key))
        code, length, first, last = table[symbol]
        st, at = self.stats, self.pos % 32
        st["codes"][key][length] += 1
        ends = st["first_last"][key].setdefault(length, [False, False])
        ends[0], ends[1] = ends[0] or first, ends[1] or last
        st["symbols"][key].add(symbol)
        n = symbol & 15
        if length >= 10:
            st["long_code_offsets"].add(at)
            st["long_code_offsets_by_length"].setdefault(length, set()).add(at)
        if length == 16 and n >= 10 and at + length + n > 32:
            st["crossings"].add(at)
        self.raw(format(code, "0%db" % length))
        if n:
            v = int(value)
            if not -(1 << n) < v < (1 << n):
                raise ValueError("jpeg_writer: %d does not fit %d bits" % (v, n))
            self.raw(format(v if v >= 0 else v + (1 << n) - 1, "0%db" % n))

    def finish(self):
        """-> (the stuffed bytes, a dict of this segment's figures); padded with 1-bits to a whole byte."""
        padding = -self.pos % 8
        s = "".join(self.bits) + "1" * padding
        plain = int(s, 2).to_bytes(len(s) // 8, "big") if s else b""
        return plain.replace(b"\xff", b"\xff\x00"), dict(bytes=len(plain), bits=self.pos, padding=padding,
                                                         stuffed=plain.count(b"\xff"), ends_stuffed=plain.endswith(b"\xff"))


def _marker(m, payload, fill):
    return b"\xff" * fill + bytes([0xFF, m]) + struct.pack(">H", len(payload) + 2) + payload


def _dqt_entry(tq, table):
    t = np.asarray(table).reshape(64)
    assert t.min() >= 1 and t.max() <= 255
    return bytes([tq]) + bytes(int(t[ZIGZAG[k]]) for k in range(64))


def _dht_entry(cls, th, spec):
    bits, values = spec
    return bytes([(cls << 4) | th]) + bytes(bits) + bytes(values)


def write_jpeg(width, height, blocks, quant, dc, ac, sampling=None, selectors=None, restart=0, dqt_layout=None, dht_layout=None,
               fill=0, rst_fill=None, eoi_fill=0, extra=(), jfif=True):
    """-> ``(file bytes, stats)``.

    ``quant`` {selector: 64 steps in natural order}, ``dc`` / ``ac`` {selector: spec}, up to four each; ``selectors``: per
    component ``(tq, td, ta)`` (default: 0 for the first, 1 for the others); ``restart``: the interval in MCUs, 0 for none (a
    DRI is written whenever it is not 0, RSTn markers only between intervals).

    Header layout.  ``dqt_layout``: a list of DQT segments, each a list of selectors or ``(selector, table)`` pairs -- a pair
    defines the selector with another table, so that a later entry can redefine it (default: one segment per table);
    ``dht_layout`` likewise, of ``("dc" | "ac", selector)`` or ``("dc" | "ac", selector, spec)``.  ``fill``: FF fill bytes in
    front of every header marker; ``rst_fill`` {interval index: fill bytes in front of the RSTn behind it}; ``eoi_fill``;
    ``extra``: ``(where, marker, payload)`` segments with ``where`` one of ``soi``, ``dqt``, ``sof``, ``dht``: behind which
    part they go.

    ``stats``: ``codes`` {("dc" | "ac", selector): counts by code length, index 0..16}; ``first_last`` {table: {length:
    [first code emitted, last code emitted]}}; ``symbols`` {table: set}; ``long_code_offsets``, the bit offsets mod 32 in the
    un-stuffed segment at which a code of 10 bits or more began (``long_code_offsets_by_length`` {length: set});
    ``crossings``, the offsets mod 32 at which a 16-bit code began whose value of 10 bits or more ended behind the next
    32-bit boundary; ``zrl``, ``eob``, ``end63`` (blocks whose coefficient 63 was written, from coefficients or by an escape
    whose runs land there), ``stuffed``; ``segments``, per restart interval ``bytes`` (un-stuffed), ``bits``, ``padding``,
    ``stuffed``, ``ends_stuffed``, ``fill``, ``first`` and ``mcus``; and what was asked for: ``mcus``, ``restart``,
    ``selectors``, ``quant``, ``dc`` and ``ac`` (the tables the data was coded with, whatever the header defined first)."""
    ncomp = 3 if sampling else 1
    assert len(blocks) == ncomp and sampling in (None, (1, 1), (2, 1), (2, 2))
    hs, vs = sampling or (1, 1)
    mw, mh, grid = block_grid(width, height, sampling)
    for comp, (bw, bh) in zip(blocks, grid):
        assert len(comp) == bw * bh, "a component of %d blocks, its grid holds %d" % (len(comp), bw * bh)
    if selectors is None:
        selectors = [(0, 0, 0)] + [(1, 1, 1)] * (ncomp - 1)
    assert len(selectors) == ncomp and len(quant) <= 4 and len(dc) <= 4 and len(ac) <= 4
    tables = {("dc", k): code_table(v) for k, v in dc.items()}
    tables.update({("ac", k): code_table(v) for k, v in ac.items()})
    stats = dict(codes={k: [0] * 17 for k in tables}, first_last={k: {} for k in tables}, symbols={k: set() for k in tables},
                 long_code_offsets=set(), long_code_offsets_by_length={}, crossings=set(), zrl=0, eob=0, end63=0, stuffed=0,
                 segments=[], mcus=mw * mh, restart=restart, selectors=[tuple(s) for s in selectors],
                 quant={k: [int(v) for v in np.asarray(t).reshape(64)] for k, t in quant.items()},
                 dc={k: (list(v[0]), list(v[1])) for k, v in dc.items()}, ac={k: (list(v[0]), list(v[1])) for k, v in ac.items()})

    # ---- the entropy-coded data
    mcus, interval = mw * mh, restart or mw * mh
    rst_fill = rst_fill or {}
    scan, m = b"", 0
    while m < mcus:
        seg, pred = _Segment(stats), [0] * ncomp
        count = min(interval, mcus - m)
        for mcu in range(m, m + count):
            my, mx = divmod(mcu, mw)
            order = [(0, (my * vs + v) * grid[0][0] + mx * hs + h) for v in range(vs) for h in range(hs)]
            order += [(c, my * mw + mx) for c in range(1, ncomp)]
            for c, at in order:
                blk = blocks[c][at]
                escape = isinstance(blk, list) and any(isinstance(x, (tuple, str)) for x in blk)
                items = blk if escape else block_pairs(np.asarray(blk).reshape(64), pred[c])
                first, i = True, 1
                for item in items:
                    if isinstance(item, str):
                        seg.raw(item)
                        continue
                    symbol, value = item
                    if first:
                        seg.symbol(("dc", selectors[c][1]), tables[("dc", selectors[c][1])], symbol, value)
                        pred[c] += int(value) if symbol & 15 else 0
                        first = False
                        continue
                    seg.symbol(("ac", selectors[c][2]), tables[("ac", selectors[c][2])], symbol, value)
                    r, s = symbol >> 4, symbol & 15
                    if symbol == ZRL:
                        stats["zrl"] += 1
                        i += 16
                    elif s == 0:
                        stats["eob"] += symbol == EOB
                    else:
                        i += r
                        stats["end63"] += i == 63
                        i += 1
        data, figures = seg.finish()
        k = len(stats["segments"])
        figures.update(first=m, mcus=count, fill=rst_fill.get(k, 0))
        stats["segments"].append(figures)
        stats["stuffed"] += figures["stuffed"]
        m += count
        scan += data
        if m < mcus:
            scan += b"\xff" * rst_fill.get(k, 0) + bytes([0xFF, 0xD0 + k % 8])

    # ---- the headers
    def extras(where):
        return b"".join(_marker(mk, payload, fill) for w, mk, payload in extra if w == where)

    out = b"\xff\xd8"
    if jfif:
        out += _marker(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00", fill)
    out += extras("soi")
    for entries in (dqt_layout if dqt_layout is not None else [[k] for k in sorted(quant)]):
        out += _marker(0xDB, b"".join(_dqt_entry(e, quant[e]) if isinstance(e, int) else _dqt_entry(*e) for e in entries), fill)
    out += extras("dqt")
    sof = struct.pack(">BHHB", 8, height, width, ncomp)
    for c in range(ncomp):
        sof += bytes([c + 1, (hs << 4 | vs) if c == 0 else 0x11, selectors[c][0]])
    out += _marker(0xC0, sof, fill) + extras("sof")
    default = [[("dc", k)] for k in sorted(dc)] + [[("ac", k)] for k in sorted(ac)]
    for entries in (dht_layout if dht_layout is not None else default):
        payload = b""
        for e in entries:
            cls, th = e[0], e[1]
            payload += _dht_entry(("dc", "ac").index(cls), th, e[2] if len(e) == 3 else (dc if cls == "dc" else ac)[th])
        out += _marker(0xC4, payload, fill)
    out += extras("dht")
    if restart:
        out += _marker(0xDD, struct.pack(">H", restart), fill)
    sos = bytes([ncomp]) + b"".join(bytes([c + 1, selectors[c][1] << 4 | selectors[c][2]]) for c in range(ncomp)) + b"\x00\x3f\x00"
    out += _marker(0xDA, sos, fill)
    return out + scan + b"\xff" * eoi_fill + b"\xff\xd9", stats
