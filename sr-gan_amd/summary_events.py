"""TensorBoard event files, written and read natively (host only: the standard library and NumPy).

What ``utility.SummaryWriter`` falls back to when tensorboardX does not import, and what a user without TensorBoard reads a
run with (``python -m srgan_amd.summary_events DIR``).  Three layers, each small enough to check by hand:

* a TFRecord frame per record: ``uint64 LE length | uint32 LE masked_crc32c(length bytes) | data | uint32 LE masked_crc32c(data)``;
* the ``Event`` / ``Summary`` messages of TensorBoard's public schema, hand-encoded (varint, fixed32 / fixed64, length-delimited);
  only the fields listed in ``FIELDS`` below exist here;
* PNG pictures written by hand (8-bit, colour type 2 or 0, filter 0, one IDAT through ``zlib``).

The byte rule for float pictures is the port's contract: ``b = uint8(floor(clamp(x, 0, 1) * 255 + 0.5))`` with NaN -> 0, that is
round to nearest, so a pixel ``k / 255`` from ``image_summaries.make_grid`` comes back as ``k``.  tensorboardX truncates instead
(``(x * 255).astype(uint8)``); it is not installed where this was written, so that difference could not be looked at.

The histogram record (``histogram_of_array``, and ``functional.tensor_histogram`` on the device with the same contract, see
``srgan_tensor_histogram`` in include/srgan_hip.h) is a dict ``{min, max, sum, sum_squares, finite_count, edges [bins + 1],
counts [bins]}`` over the FINITE elements; its proto gets ``num = finite_count``, ``bucket_limit = edges[1:]``, ``bucket = counts``.
Out of scope: audio, text, embedding and graph summaries, TensorBoard's exponential default buckets, NumPy's ``'auto'`` bins."""
import os
import socket
import struct
import sys
import time
import zlib

import numpy as np

# ---------------------------------------------------------------------------------------------------------------- CRC32C
_CRC_TABLE = []
for _byte in range(256):
    _crc = _byte
    for _ in range(8):
        _crc = (_crc >> 1) ^ 0x82F63B78 if _crc & 1 else _crc >> 1
    _CRC_TABLE.append(_crc)
del _byte, _crc


def crc32c(data, crc=0):
    """CRC-32C (Castagnoli, reflected polynomial 0x82F63B78) of ``data``, continuing from ``crc``: ``crc32c(a + b) ==
    crc32c(b, crc32c(a))``.  Pure Python, a 256-entry table: about 0.16 s per MB (profiles/summary_events.md)."""
    crc ^= 0xffffffff
    table = _CRC_TABLE
    for byte in bytes(data):
        crc = table[(crc ^ byte) & 0xff] ^ (crc >> 8)
    return crc ^ 0xffffffff


def masked_crc32c(data):
    """The TFRecord form of the checksum: rotated right by 15 and offset."""
    c = crc32c(data)
    return (((c >> 15) | (c << 17)) + 0xa282ead8) & 0xffffffff


def frame_record(data):
    header = struct.pack('<Q', len(data))
    return header + struct.pack('<I', masked_crc32c(header)) + data + struct.pack('<I', masked_crc32c(data))


# ------------------------------------------------------------------------------------------------------------ wire format
VARINT, FIXED64, BYTES, FIXED32 = 0, 1, 2, 5

# message -> {field number: (name, kind)}; kind: double / float / int64 / int32 / string / bytes / packed_double, or a message name
FIELDS = {
    'Event': {1: ('wall_time', 'double'), 2: ('step', 'int64'), 3: ('file_version', 'string'), 5: ('summary', 'Summary')},
    'Summary': {1: ('value', 'Value')},                                            # repeated
    'Value': {1: ('tag', 'string'), 2: ('simple_value', 'float'), 4: ('image', 'Image'), 5: ('histo', 'HistogramProto')},
    'Image': {1: ('height', 'int32'), 2: ('width', 'int32'), 3: ('colorspace', 'int32'), 4: ('encoded_image_string', 'bytes')},
    'HistogramProto': {1: ('min', 'double'), 2: ('max', 'double'), 3: ('num', 'double'), 4: ('sum', 'double'),
                       5: ('sum_squares', 'double'), 6: ('bucket_limit', 'packed_double'), 7: ('bucket', 'packed_double')},
}


def _varint(value):
    value &= 0xffffffffffffffff           # a negative int64 is its 64-bit two's complement: ten bytes
    out = bytearray()
    while value > 0x7f:
        out.append((value & 0x7f) | 0x80)
        value >>= 7
    out.append(value)
    return bytes(out)


def _key(field, wire_type):
    return _varint((field << 3) | wire_type)


def _delimited(field, payload):
    return _key(field, BYTES) + _varint(len(payload)) + payload


def _double(field, value):
    return _key(field, FIXED64) + struct.pack('<d', value)


def _packed_doubles(field, values):
    values = np.ascontiguousarray(values, dtype='<f8').reshape(-1)
    return _delimited(field, values.tobytes()) if values.size else b''


def encode_image(height, width, channels, png):
    return _key(1, VARINT) + _varint(height) + _key(2, VARINT) + _varint(width) + _key(3, VARINT) + _varint(channels) + \
        _delimited(4, png)


def encode_histogram(record):
    """``HistogramProto`` of a histogram record: num = finite_count, bucket_limit = edges[1:], bucket = counts."""
    return _double(1, float(record['min'])) + _double(2, float(record['max'])) + _double(3, float(record['finite_count'])) + \
        _double(4, float(record['sum'])) + _double(5, float(record['sum_squares'])) + \
        _packed_doubles(6, np.asarray(record['edges'], dtype=np.float64)[1:]) + _packed_doubles(7, record['counts'])


def encode_value(tag, simple_value=None, image=None, histo=None):
    """``Summary.Value``: the tag and ONE of a float, an encoded ``Image`` and an encoded ``HistogramProto``."""
    out = _delimited(1, tag.encode('utf-8'))
    if simple_value is not None:
        out += _key(2, FIXED32) + struct.pack('<f', simple_value)
    if image is not None:
        out += _delimited(4, image)
    if histo is not None:
        out += _delimited(5, histo)
    return out


def encode_event(wall_time, step=0, file_version=None, values=None):
    """``Event``: ``values`` is a list of encoded ``Summary.Value``; a zero step is left out, as proto3 leaves defaults out."""
    out = _double(1, wall_time)
    if step:
        out += _key(2, VARINT) + _varint(int(step))
    if file_version is not None:
        out += _delimited(3, file_version.encode('utf-8'))
    if values is not None:
        out += _delimited(5, b''.join(_delimited(1, value) for value in values))
    return out


def _read_varint(data, at):
    value, shift = 0, 0
    while True:
        if at >= len(data) or shift > 63:
            raise ValueError('malformed varint')
        byte = data[at]
        at += 1
        value |= (byte & 0x7f) << shift
        shift += 7
        if not byte & 0x80:
            return value, at


def _fields(data):
    """(field number, wire type, value) of every field of a message, in order; value: an int, or the raw bytes."""
    at = 0
    while at < len(data):
        key, at = _read_varint(data, at)
        field, wire_type = key >> 3, key & 7
        if wire_type == VARINT:
            value, at = _read_varint(data, at)
        elif wire_type in (FIXED64, FIXED32):
            width = 8 if wire_type == FIXED64 else 4
            value, at = data[at:at + width], at + width
        elif wire_type == BYTES:
            length, at = _read_varint(data, at)
            value, at = data[at:at + length], at + length
        else:
            raise ValueError(f'wire type {wire_type} (field {field}) cannot be skipped')
        if at > len(data):
            raise ValueError(f'field {field} runs past the end of its message')
        yield field, wire_type, value


_WIRE_TYPES = {'double': FIXED64, 'float': FIXED32, 'int64': VARINT, 'int32': VARINT, 'string': BYTES, 'bytes': BYTES,
               'packed_double': BYTES}


def decode_message(name, data):
    """A dict of the known fields of message ``name`` (``Summary.value`` as a list); unknown fields are skipped by wire type."""
    out = {'value': []} if name == 'Summary' else {}
    for field, wire_type, value in _fields(bytes(data)):
        known = FIELDS[name].get(field)
        if known is None or wire_type != _WIRE_TYPES.get(known[1], BYTES):
            continue
        key, kind = known
        if kind == 'double':
            value = struct.unpack('<d', value)[0]
        elif kind == 'float':
            value = struct.unpack('<f', value)[0]
        elif kind in ('int64', 'int32'):
            value = value - (1 << 64) if value >= 1 << 63 else value
        elif kind == 'string':
            value = value.decode('utf-8')
        elif kind == 'packed_double':
            value = np.frombuffer(value, dtype='<f8').astype(np.float64)
            value = np.concatenate([out[key], value]) if key in out else value
        elif kind != 'bytes':
            value = decode_message(kind, value)
        if name == 'Summary':
            out['value'].append(value)
        else:
            out[key] = value
    return out


# -------------------------------------------------------------------------------------------------------------------- PNG
def image_bytes(image):
    """``uint8 [H, W, channels]`` (channels 1 or 3) of a picture: ``[3, H, W]``, ``[1, H, W]`` or ``[H, W]`` floats through the
    byte rule ``floor(clamp(x, 0, 1) * 255 + 0.5)`` with NaN -> 0 (evaluated in float64, where it is exact for float32 input:
    round to nearest, ties up), or ``[H, W, 3]`` / ``[H, W]`` uint8 as they are."""
    image = np.asarray(image)
    if image.dtype == np.uint8:
        if image.ndim == 2:
            image = image[:, :, None]
        if image.ndim != 3 or image.shape[2] not in (1, 3):
            raise ValueError(f'a uint8 picture is [H, W, 3] or [H, W], not {image.shape}')
        return np.ascontiguousarray(image)
    if not np.issubdtype(image.dtype, np.floating):
        raise ValueError(f'a picture is float or uint8, not {image.dtype}')
    if image.ndim == 2:
        image = image[None]
    if image.ndim != 3 or image.shape[0] not in (1, 3):
        raise ValueError(f'a float picture is [3, H, W], [1, H, W] or [H, W], not {image.shape}')
    wide = image.astype(np.float64)
    wide = np.clip(np.where(np.isnan(wide), 0.0, wide), 0.0, 1.0)
    return np.ascontiguousarray(np.floor(wide * 255.0 + 0.5).astype(np.uint8).transpose(1, 2, 0))


def _png_chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xffffffff)


def encode_png(pixels):
    """PNG of ``uint8 [H, W, 1 or 3]``: 8 bits, colour type 0 (grey) or 2 (RGB), filter 0 on every row, one IDAT."""
    height, width, channels = pixels.shape
    if height < 1 or width < 1:
        raise ValueError('an empty picture cannot be a PNG')
    rows = np.empty((height, 1 + width * channels), dtype=np.uint8)
    rows[:, 0] = 0
    rows[:, 1:] = pixels.reshape(height, width * channels)
    header = struct.pack('>IIBBBBB', width, height, 8, 2 if channels == 3 else 0, 0, 0, 0)
    return b'\x89PNG\r\n\x1a\n' + _png_chunk(b'IHDR', header) + _png_chunk(b'IDAT', zlib.compress(rows.tobytes())) + \
        _png_chunk(b'IEND', b'')


# ----------------------------------------------------------------------------------------------------------- histograms
def check_bins(bins):
    if isinstance(bins, str):             # the reference wrapper's default is 'auto' (utility.py:35); NumPy's rule is out of scope
        return 30
    if int(bins) != bins or not 1 <= bins <= 1024:
        raise ValueError(f'bins is an integer in [1, 1024], not {bins!r}')
    return int(bins)


def histogram_record(out, bins):
    """The record dict of ``out`` = the ``5 + (bins + 1) + bins`` doubles of ``srgan_tensor_histogram``."""
    out = np.asarray(out, dtype=np.float64)
    return {'min': float(out[0]), 'max': float(out[1]), 'sum': float(out[2]), 'sum_squares': float(out[3]),
            'finite_count': float(out[4]), 'edges': out[5:6 + bins].copy(), 'counts': out[6 + bins:6 + 2 * bins].copy()}


def histogram_of_array(array, bins=30):
    """The contract of ``srgan_tensor_histogram`` (include/srgan_hip.h) in NumPy float64, for host arrays: only finite elements
    count; min / max with a zero reported as +0.0; sums in float64 started from +0.0; edges ``lo + i * ((hi - lo) / bins)`` with
    ``edge_bins = hi`` exactly and ``lo, hi = min -+ 0.5`` when ``min == max``; an element belongs to the largest ``i <= bins - 1``
    with ``edge_i <= x``.  No finite element: all zeros.  (float32 input converts exactly; the sums' order is NumPy's.)"""
    bins = check_bins(bins)
    values = np.asarray(array)
    if values.dtype not in (np.float32, np.float64):
        values = values.astype(np.float32)                # what the device kernel sees of such a tensor
    values = values.reshape(-1).astype(np.float64)
    values = values[np.isfinite(values)]
    out = np.zeros(5 + 2 * bins + 1, dtype=np.float64)
    if values.size:
        low, high = float(values.min()) + 0.0, float(values.max()) + 0.0
        out[:5] = low, high, float(values.sum()) + 0.0, float((values * values).sum()) + 0.0, values.size
        if low == high:
            low, high = low - 0.5, high + 0.5
        edges = low + np.arange(bins + 1, dtype=np.float64) * ((high - low) / bins)
        edges[bins] = high
        index = np.clip(np.searchsorted(edges, values, side='right') - 1, 0, bins - 1)
        out[5:6 + bins] = edges
        out[6 + bins:] = np.bincount(index, minlength=bins)
    return histogram_record(out, bins)


# ------------------------------------------------------------------------------------------------------------- the writer
_writers_of_this_process = 0


class EventFileWriter:
    """One event file ``events.out.tfevents.<10-digit seconds>.<hostname>.<pid>.<n>`` in ``log_dir`` (made when missing); ``n``
    counts the writers of this process, so two writers of one directory never share a file.  The first record is the version
    event.  Records reach the operating system at ``flush()`` and ``close()``; a write after ``close()`` raises."""

    def __init__(self, log_dir):
        global _writers_of_this_process
        os.makedirs(log_dir, exist_ok=True)
        now = time.time()
        name = 'events.out.tfevents.%010d.%s.%d.%d' % (int(now), socket.gethostname(), os.getpid(), _writers_of_this_process)
        _writers_of_this_process += 1
        self.path = os.path.join(log_dir, name)
        self._file = open(self.path, 'wb')
        self.encode_seconds = 0.0          # host time spent encoding and framing, for profiles/summary_events.md
        self._write(encode_event(now, file_version='brain.Event:2'))
        self.flush()

    def _write(self, event):
        if self._file is None:
            raise ValueError(f'{self.path} is closed')
        self._file.write(frame_record(event))

    def _add(self, value, step, wall_time):
        self._write(encode_event(time.time() if wall_time is None else wall_time, step, values=[value]))

    def add_scalar(self, tag, value, step, wall_time=None):
        start = time.perf_counter()
        self._add(encode_value(tag, simple_value=float(value)), step, wall_time)
        self.encode_seconds += time.perf_counter() - start

    def add_image(self, tag, image, step, wall_time=None):
        """``image``: see ``image_bytes`` for the accepted shapes and the byte rule."""
        start = time.perf_counter()
        pixels = image_bytes(image)
        height, width, channels = pixels.shape
        self._add(encode_value(tag, image=encode_image(height, width, channels, encode_png(pixels))), step, wall_time)
        self.encode_seconds += time.perf_counter() - start

    def add_histogram(self, tag, record, step, wall_time=None):
        """``record``: a histogram record (``histogram_of_array`` / ``functional.tensor_histogram``)."""
        start = time.perf_counter()
        self._add(encode_value(tag, histo=encode_histogram(record)), step, wall_time)
        self.encode_seconds += time.perf_counter() - start

    def flush(self):
        if self._file is not None:
            self._file.flush()

    def close(self):
        if self._file is not None:
            self._file.close()
            self._file = None


# ------------------------------------------------------------------------------------------------------------- the reader
def read_events(path, allow_truncated=False):
    """One dict per record of an event file: ``wall_time``, ``step``, and ``file_version`` or ``values`` = a list of ``{tag,
    simple_value | image | histo}``; an image is ``(height, width, channels, png_bytes)``, a histogram the dict of its proto's
    fields.  A length or data checksum that does not match raises ``ValueError`` naming the record's byte offset; so does a
    final record that is cut off, unless ``allow_truncated`` (a file that is still being written)."""
    with open(path, 'rb') as handle:
        data = handle.read()
    at = 0
    while at < len(data):
        header = data[at:at + 12]
        if len(header) == 12:
            length, length_crc = struct.unpack('<QI', header)
            if masked_crc32c(header[:8]) != length_crc:
                raise ValueError(f'{path}: length checksum mismatch in the record at byte offset {at}')
        if len(header) < 12 or at + 12 + length + 4 > len(data):
            if allow_truncated:
                return
            raise ValueError(f'{path}: the record at byte offset {at} is cut off')
        payload = data[at + 12:at + 12 + length]
        if masked_crc32c(payload) != struct.unpack('<I', data[at + 12 + length:at + 16 + length])[0]:
            raise ValueError(f'{path}: data checksum mismatch in the record at byte offset {at}')
        at += 16 + length
        event = decode_message('Event', payload)
        record = {'wall_time': event.get('wall_time', 0.0), 'step': event.get('step', 0)}
        if 'file_version' in event:
            record['file_version'] = event['file_version']
        if 'summary' in event:
            record['values'] = values = []
            for value in event['summary']['value']:
                entry = {'tag': value.get('tag', '')}
                if 'simple_value' in value:
                    entry['simple_value'] = value['simple_value']
                if 'image' in value:
                    image = value['image']
                    entry['image'] = (image.get('height', 0), image.get('width', 0), image.get('colorspace', 0),
                                      image.get('encoded_image_string', b''))
                if 'histo' in value:
                    histo = {'min': 0.0, 'max': 0.0, 'num': 0.0, 'sum': 0.0, 'sum_squares': 0.0,
                             'bucket_limit': np.zeros(0), 'bucket': np.zeros(0)}
                    histo.update(value['histo'])
                    entry['histo'] = histo
                values.append(entry)
        yield record


def _name_order(name):
    """The sort key of an event file's name: its fields in order, the numbers (seconds, pid, writer count) compared as numbers,
    so that writer 10 of a process comes after its writer 8."""
    fields = name[len('events.out.tfevents.'):].split('.')
    if len(fields) >= 4 and fields[0].isdigit() and fields[-2].isdigit() and fields[-1].isdigit():
        return (0, int(fields[0]), '.'.join(fields[1:-2]), int(fields[-2]), int(fields[-1]))
    return (1, 0, name, 0, 0)             # a file some other writer named: after ours, by name


def event_files(directory):
    """The event files of ``directory`` in name order (numbers as numbers): the order they were opened in, since a name starts
    with the time and ends with the count of the process's writers."""
    names = [name for name in os.listdir(directory) if name.startswith('events.out.tfevents.')]
    return [os.path.join(directory, name) for name in sorted(names, key=_name_order)]


def scalars(directory, allow_truncated=False):
    """``{tag: [(step, value)]}`` over all event files of ``directory`` in name order, each file's records in file order."""
    out = {}
    for path in event_files(directory):
        for record in read_events(path, allow_truncated=allow_truncated):
            for value in record.get('values', ()):
                if 'simple_value' in value:
                    out.setdefault(value['tag'], []).append((record['step'], value['simple_value']))
    return out


def main(arguments=None):
    """``python -m srgan_amd.summary_events DIR``: the scalars of a run as ``tag<TAB>step<TAB>value`` lines, tags in name order."""
    arguments = sys.argv[1:] if arguments is None else arguments
    if len(arguments) != 1:
        print('usage: python -m srgan_amd.summary_events DIRECTORY', file=sys.stderr)
        return 2
    for tag, points in sorted(scalars(arguments[0], allow_truncated=True).items()):
        for step, value in points:
            print('%s\t%d\t%.9g' % (tag, step, value))
    return 0


if __name__ == '__main__':
    sys.exit(main())
