"""Plain numpy references for the list-column decode kernels.

Shared by the GPU kernel tests (oracle for ``list_count_batch`` /
``list_assemble_batch``) and the CPU dry run, whose stub extension runs
these in place of the kernels so the decoder's Python orchestration is
checked value for value without a GPU.  Written entry by entry on purpose:
nothing here shares structure with the wave-parallel kernels.
"""

import numpy as np


def rle_hybrid_decode_reference(buf, start, end, bit_width, n_values):
    """Parquet RLE / bit-packed hybrid stream ``buf[start:end]`` -> the
    first ``n_values`` values (int32)."""
    data = bytes(bytearray(buf[start:end]))
    out, pos = [], 0
    while len(out) < n_values and pos < len(data):
        header, shift = 0, 0
        while True:
            b = data[pos]
            pos += 1
            header |= (b & 0x7f) << shift
            shift += 7
            if not b & 0x80:
                break
        if header & 1:
            nbytes = (header >> 1) * bit_width
            bits = int.from_bytes(data[pos:pos + nbytes], 'little')
            pos += nbytes
            out.extend((bits >> (i * bit_width)) & ((1 << bit_width) - 1)
                       for i in range((header >> 1) * 8))
        else:
            nbytes = (bit_width + 7) // 8
            out.extend([int.from_bytes(data[pos:pos + nbytes], 'little')] *
                       (header >> 1))
            pos += nbytes
    assert len(out) >= n_values, 'level stream too short'
    return np.asarray(out[:n_values], dtype=np.int32)


def assemble_lists_reference(rep, dfl, page_nval, val_buf, val_start,
                             val_end, esize, fill, def_slot, max_def,
                             list_nullable, n_rows):
    """Repetition / definition levels + per-page PLAIN value spans ->
    ``offsets`` [n_rows + 1], ``values`` (uint8 [slots * esize]),
    ``elem_valid`` [slots], ``list_valid`` [n_rows], per-page ``counts``
    [pages, 3] (rows, slots, values) and per-page ``status`` (0 ok; 1 the
    first entry continues a row; 2 row index past ``n_rows``; 3 value span
    too short)."""
    n_pages = len(page_nval)
    offsets = np.zeros(n_rows + 1, dtype=np.int64)
    list_valid = np.zeros(n_rows, dtype=np.uint8)
    counts = np.zeros((n_pages, 3), dtype=np.int64)
    status = np.zeros(n_pages, dtype=np.int32)
    fill_bytes = [(fill >> (8 * b)) & 0xff for b in range(esize)]
    values, elem_valid = [], []
    row, entry = 0, 0
    for page in range(n_pages):
        pos = int(val_start[page])
        for _ in range(int(page_nval[page])):
            r, d = int(rep[entry]), int(dfl[entry])
            if entry == 0 and r != 0:
                status[page] = 1
            if r == 0:
                counts[page, 0] += 1
                if row < n_rows:
                    offsets[row] = len(elem_valid)
                    list_valid[row] = 0 if (list_nullable and d == 0) else 1
                else:
                    status[page] = 2
                row += 1
            if d >= def_slot:
                counts[page, 1] += 1
                if d == max_def:
                    counts[page, 2] += 1
                    if pos + esize <= int(val_end[page]):
                        values.extend(val_buf[pos:pos + esize].tolist())
                        elem_valid.append(1)
                    else:  # the kernel skips the access: slot undefined
                        status[page] = 3
                        values.extend([0] * esize)
                        elem_valid.append(1)
                    pos += esize
                else:
                    values.extend(fill_bytes)
                    elem_valid.append(0)
            entry += 1
    offsets[n_rows] = len(elem_valid)
    return dict(offsets=offsets, values=np.asarray(values, dtype=np.uint8),
                elem_valid=np.asarray(elem_valid, dtype=np.uint8),
                list_valid=list_valid, counts=counts, status=status)
