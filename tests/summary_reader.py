"""The event-file reader of the summary tests: its own record framing and protocol-buffer wire decode, written against the
format (m4depth_amd/summaries.py's docstring) and sharing nothing with the writer but crc32c."""
import io
import struct

import numpy as np

from m4depth_amd.tf_checkpoint import crc32c


def mask(c):
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def read_records(blob):
    """The payloads of an event file; raises ValueError on a bad length or data checksum or a truncated record."""
    pos, out = 0, []
    while pos < len(blob):
        if pos + 12 > len(blob):
            raise ValueError("truncated record header")
        (length,), (len_crc,) = struct.unpack_from("<Q", blob, pos), struct.unpack_from("<I", blob, pos + 8)
        if mask(crc32c(blob[pos:pos + 8])) != len_crc:
            raise ValueError(f"length checksum mismatch at offset {pos}")
        if pos + 12 + length + 4 > len(blob):
            raise ValueError("truncated record")
        payload = blob[pos + 12:pos + 12 + length]
        if mask(crc32c(payload)) != struct.unpack_from("<I", blob, pos + 12 + length)[0]:
            raise ValueError(f"data checksum mismatch at offset {pos}")
        out.append(payload)
        pos += 12 + length + 4
    return out


def decode_fields(buf):
    """Protocol-buffer wire decode: [(field number, wire type, value)]; varints as ints, fixed fields and length-delimited
    fields as bytes."""
    pos, out = 0, []

    def varint():
        nonlocal pos
        shift = v = 0
        while True:
            b = buf[pos]
            pos += 1
            v |= (b & 0x7F) << shift
            shift += 7
            if not b & 0x80:
                return v
    while pos < len(buf):
        key = varint()
        field, wt = key >> 3, key & 7
        if wt == 0:
            out.append((field, wt, varint()))
        elif wt in (1, 5):
            size = 8 if wt == 1 else 4
            out.append((field, wt, bytes(buf[pos:pos + size])))
            pos += size
        elif wt == 2:
            size = varint()
            out.append((field, wt, bytes(buf[pos:pos + size])))
            pos += size
        else:
            raise ValueError(f"wire type {wt}")
        if pos > len(buf):
            raise ValueError("field runs past the message")
    return out


def decode_event(payload):
    """{'wall_time', 'step', 'file_version', 'values': [{'tag', 'simple_value_bits' | 'image': {...}}]}"""
    ev = {"step": 0, "values": []}
    for field, wt, v in decode_fields(payload):
        if (field, wt) == (1, 1):
            ev["wall_time"] = struct.unpack("<d", v)[0]
        elif (field, wt) == (2, 0):
            ev["step"] = v
        elif (field, wt) == (3, 2):
            ev["file_version"] = v.decode()
        elif (field, wt) == (5, 2):
            for f2, w2, raw in decode_fields(v):
                assert (f2, w2) == (1, 2)
                val = {}
                for f3, w3, x in decode_fields(raw):
                    if (f3, w3) == (1, 2):
                        val["tag"] = x.decode()
                    elif (f3, w3) == (2, 5):
                        val["simple_value_bits"] = struct.unpack("<I", x)[0]
                    elif (f3, w3) == (4, 2):
                        names = {1: "height", 2: "width", 3: "colorspace", 4: "png"}
                        val["image"] = {names[f4]: y for f4, _, y in decode_fields(x)}
                    else:
                        raise ValueError(f"Summary.Value field {f3} / wire type {w3}")
                ev["values"].append(val)
        else:
            raise ValueError(f"Event field {field} / wire type {wt}")
    return ev


def read_events(path):
    with open(path, "rb") as fh:
        return [decode_event(p) for p in read_records(fh.read())]


def png_pixels(png):
    from PIL import Image
    with Image.open(io.BytesIO(png)) as im:
        return np.asarray(im)


def bits(v):
    return int(np.float32(v).view(np.uint32))
