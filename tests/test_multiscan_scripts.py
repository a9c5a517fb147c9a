"""Every scan script of a three-component baseline frame, and tables defined between its scans (beyond the reference, which stops
after the first scan; DESIGN s9).

A frame of three components can be coded as two or three scans, each carrying one component (non-interleaved, T.81 A.2.2) or an
interleaved pair (A.2.3): 12 scripts (jpegwriter.SCRIPTS).  jpegwriter.script_twins re-encodes the quantised coefficients of an
interleaved layout_jpeg file under each, so every twin has the source's picture.  Pillow (libjpeg), where installed, pins the writer
independently of the oracle: its decode of a twin equals its decode of the source exactly.

T.81 allows DQT, DHT and DRI segments between scans.  A component's quantisation table is the one its slot holds when the scan that
carries it starts (libjpeg: latch_quant_tables); a slot redefined later does not change it, and a slot not defined by then is an
error.  mjx_parse and the oracle's ext_multiscan keep that rule.

GPU tests compare with the GPU picture of the interleaved source bit for bit, and collect every failing case before they assert.
"""
import functools
import io

import numpy as np
import pytest

import jpegwriter as jw
import oracle_binding as orc_mod
import test_sampling_layouts as sl

SCRIPTS = jw.SCRIPTS
# planar_ok's pair branch with components of more than one block: consecutive or not, blocks per MCU a power of two or not
PAIR_LAYOUTS = ["Y11_Cb11_Cr11", "Y22_Cb11_Cr11", "Y21_Cb11_Cr11", "Y12_Cb11_Cr11", "Y22_Cb22_Cr11", "Y21_Cb21_Cr11",
                "Y21_Cb12_Cr11", "Y11_Cb22_Cr11", "Y11_Cb11_Cr22", "Y22_Cb22_Cr22"]
TABLE_LAYOUTS = ["Y22_Cb11_Cr11", "Y11_Cb11_Cr11", "Y22_Cb22_Cr11", "Y21_Cb12_Cr12"]
TABLE_SIZES = [(37, 29), (333, 217)]
DQT_CASES = ["after", "split", "tail"]
RESTARTS = [(3, 0, 5), (0, 7, 1)]         # per scan (cut to the script's scans): script k takes RESTARTS[k % 2]


def oracle_ms(data):
    return orc_mod.decode(data, layout=orc_mod.LAYOUT_STD, ext_1bit=True, ext_dri=True, ext_multiscan=True)


@functools.lru_cache(maxsize=None)
def twins(lname, w, h):
    """the twins of layout_file(lname, w, h), in SCRIPTS order"""
    d = sl.data_of(lname, w, h)
    return tuple(jw.script_twins(d, sl.oracle_std(d), SCRIPTS))


def dqt_scripts(dqt):
    """'split' needs Cb and Cr in scans of their own"""
    return [s for s in SCRIPTS if dqt != "split" or "Cb Cr" not in s]


@functools.lru_cache(maxsize=None)
def dqt_twins(lname, w, h, dqt):
    """-> (source, twins of dqt_scripts(dqt)); 'split' starts from a source with Cb and Cr on slots of their own"""
    d = sl.data_of(lname, w, h, "three" if dqt == "split" else "split")
    return d, tuple(jw.script_twins(d, sl.oracle_std(d), dqt_scripts(dqt), dqt=dqt))


@functools.lru_cache(maxsize=None)
def table_twin(lname, w, h, k):
    """script k with per-scan Huffman tables, per-scan restart intervals and COM / APP1 between the scans"""
    d = sl.data_of(lname, w, h)
    return jw.script_twin(d, sl.oracle_std(d), SCRIPTS[k], tables="per_scan", restart=scan_restarts(k), markers=True)


def scan_restarts(k):
    return list(RESTARTS[k % 2][:len(jw.parse_script(SCRIPTS[k]))])


def pillow(data):
    """Pillow's RGB, the OSError it raises, or None without Pillow"""
    try:
        from PIL import Image
    except ImportError:
        return None
    try:
        return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    except OSError as e:
        return e


def same_pillow(got, want):
    return got is None or (isinstance(got, np.ndarray) and isinstance(want, np.ndarray) and np.array_equal(got, want))


def comp_tables(mjx, data):
    """-> ([quantisation table of each component, frame order], mjx_validate's status) as mjx_parse gives them"""
    s = mjx.ParsedScan(data)
    try:
        d = s.desc
        return [list(d.qt[d.comp[c].tq]) for c in range(3)], s.validate()
    finally:
        s.close()


def scan_units(lname, w, h, cs):
    """restart units of a scan of components cs: blocks of the component's own grid, or the frame's MCUs for a pair"""
    hv = sl.parse_name(lname)
    hmax, vmax = max(a for a, _ in hv), max(b for _, b in hv)
    cdiv = lambda a, b: -(-a // b)
    if len(cs) == 2:
        return cdiv(w, 8 * hmax) * cdiv(h, 8 * vmax)
    a, b = hv[cs[0]]
    return cdiv(cdiv(w * a, hmax), 8) * cdiv(cdiv(h * b, vmax), 8)


def scan_dhts(data):
    """[{(class, slot): (bits, vals)} of the DHT segments between the previous SOS and this one] per SOS of the file"""
    out, tabs, i = [], {}, 2
    while i + 4 <= len(data) and data[i + 1] != 0xd9:
        m, ln = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        p = data[i + 4:i + 2 + ln]
        i += 2 + ln
        if m == 0xc4:
            tabs.update(jw.tables_from_jpeg(b"\xff\xd8" + data[i - 2 - ln:i]))
        if m == 0xda:
            out.append(tabs)
            tabs = {}
            while not (data[i] == 0xff and data[i + 1] != 0 and not 0xd0 <= data[i + 1] <= 0xd7):
                i += 1
    return out


def planar_direct(lname, w, script, scale):
    """planar_ok (mjx_api.hip) for a script twin decoded alone without keep_coefs: the tile rule of sl.planar_direct, where a
    single-component scan gives its v block rows per MCU and an interleaved pair one -- when its blocks per MCU are a power of two
    and its two components are consecutive in frame order; otherwise the picture is gathered.  (planar_ok also checks that the
    pair's MCU grid is the picture's; it always is: ceil(ceil(W h / Hmax) / 8 h) = ceil(W / 8 Hmax).)"""
    hv = sl.parse_name(lname)
    kinds = 0
    for cs in jw.parse_script(script):
        if len(cs) == 1:
            kinds += hv[cs[0]][1]
            continue
        pb = sum(hv[c][0] * hv[c][1] for c in cs)
        if pb & (pb - 1) or cs[1] != cs[0] + 1:
            return False
        kinds += 1
    return sl.planar_fits(hv, w, scale, kinds)


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_scripts_and_the_direct_path_rule():
    """The 12 scripts are distinct and carry every component once, in two or three scans; for one scan per component in frame
    order planar_direct is the rule test_sampling_layouts already checks."""
    plans = [jw.parse_script(s) for s in SCRIPTS]
    assert len({str(p) for p in plans}) == 12
    assert all(len(p) in (2, 3) and sorted(sum(p, [])) == [0, 1, 2] for p in plans)
    assert sum(len(p) == 2 for p in plans) == 6
    for n in sl.NAMES:
        for w, _ in sl.TWIN_SIZES:
            for s in (1, 2, 8):
                assert planar_direct(n, w, "Y;Cb;Cr", s) == sl.planar_direct(n, w, s), (n, w, s)


@pytest.mark.parametrize("lname", sl.NAMES)
def test_every_script_decodes_to_the_source_picture(mjx, lname):
    """At every twin size: the oracle decodes every twin to the interleaved source's picture; Pillow decodes every twin to its own
    picture of the source exactly; mjx_parse lists the scans as parts in script order, and mjx_validate accepts every twin at every
    scale.  Pillow refuses the source of the 12-block MCU (T.81 B.2.3: at most 10 blocks in one scan) and decodes its twins, whose
    scans have at most 8: there every script gives Pillow the same picture, near the oracle's."""
    bad = []
    for w, h in sl.TWIN_SIZES:
        d = sl.data_of(lname, w, h)
        want, pil_src, pil_first = sl.oracle_std(d).rgb, pillow(d), None
        for script, tw in zip(SCRIPTS, twins(lname, w, h)):
            case = (w, h, script)
            if not np.array_equal(oracle_ms(tw).rgb, want):
                bad.append(case + ("oracle",))
            s = mjx.ParsedScan(tw)
            try:
                dd = s.desc
                parts = [[dd.parts[k].comp[q] for q in range(dd.parts[k].ncomp)] for k in range(dd.n_parts)]
                if parts != jw.parse_script(script):
                    bad.append(case + ("parts", parts))
                st = [s.validate(scale=k) for k in (1, 2, 4, 8)]
                if st != [mjx.OK] * 4:
                    bad.append(case + ("validate", st))
            finally:
                s.close()
            p = pillow(tw)
            if isinstance(pil_src, OSError):
                assert sum(a * b for a, b in sl.parse_name(lname)) > 10, lname
                if pil_first is None and isinstance(p, np.ndarray):
                    pil_first = p
                    if np.abs(p.astype(np.int32) - want.astype(np.int32)).mean() >= 6.0:
                        bad.append(case + ("pillow far from the oracle",))
                ok = same_pillow(p, pil_first)
            else:
                ok = same_pillow(p, pil_src)
            if not ok:
                bad.append(case + ("pillow", p if isinstance(p, OSError) else None))
    assert bad == [], bad


@pytest.mark.parametrize("dqt", DQT_CASES)
def test_quantisation_tables_are_latched_when_the_scan_starts(mjx, dqt):
    """(a) 'after': a slot redefined as soon as all its components are scanned; (b) 'split': Cb and Cr on one slot number, defined
    with each one's own table right before its scan; (c) 'tail': every slot redefined behind the last scan.  Each component keeps
    the table its slot held when its scan started: mjx_parse's desc gives it the table it was quantised with, and the oracle and
    Pillow give the source's picture.  (Were the last DQT of the file to hold for every component, each of these files would
    decode to another picture.)"""
    bad = []
    for lname in TABLE_LAYOUTS:
        for w, h in TABLE_SIZES:
            d, tws = dqt_twins(lname, w, h, dqt)
            want, pil_src = sl.oracle_std(d).rgb, pillow(d)
            src_tables, _ = comp_tables(mjx, d)
            if dqt == "split":
                assert len({str(t) for t in src_tables}) == 3
            for script, tw in zip(dqt_scripts(dqt), tws):
                case = (lname, w, h, script)
                tabs, st = comp_tables(mjx, tw)
                if tabs != src_tables or st != mjx.OK:
                    bad.append(case + ("desc", st))
                if not np.array_equal(oracle_ms(tw).rgb, want):
                    bad.append(case + ("oracle",))
                if not same_pillow(pillow(tw), pil_src):
                    bad.append(case + ("pillow",))
    assert bad == [], bad


def test_a_table_defined_after_its_scan_started_is_refused(mjx):
    """The slot of the first scan's first component is defined only behind that scan: mjx_parse says MJX_ERR_MISSING_TABLE, the
    oracle gives its missing-table panic, and Pillow (libjpeg) refuses the file too.  Defined in front, the same file decodes."""
    d = sl.data_of("Y22_Cb11_Cr11", 333, 217)
    late = jw.script_twins(d, sl.oracle_std(d), SCRIPTS, dqt="late")
    for script, tw in zip(SCRIPTS, late):
        with pytest.raises(mjx.MjxError) as e:
            mjx.ParsedScan(tw)
        assert e.value.code == mjx.ERR_MISSING_TABLE, script
        with pytest.raises(orc_mod.OracleError) as e:
            oracle_ms(tw)
        assert e.value.code == orc_mod.ERR_REF_PANIC and "quantization" in str(e.value), script
        p = pillow(tw)
        assert p is None or isinstance(p, OSError), script
    assert np.array_equal(oracle_ms(twins("Y22_Cb11_Cr11", 333, 217)[0]).rgb, sl.oracle_std(d).rgb)


@pytest.mark.parametrize("lname", TABLE_LAYOUTS)
def test_per_scan_tables_and_restart_intervals_are_parsed_into_parts(mjx, lname):
    """tables='per_scan': no DHT in front of the frame, a DHT of K.2 tables for each scan right before its SOS on slots 0 and 1;
    restart intervals per scan, switched off for one of them; COM and APP1 segments between the scans.  Every part carries the
    tables and the interval in force at its SOS, one restart offset per further interval; the oracle and Pillow give the source's
    picture, and mjx_validate accepts the file."""
    bad = []
    for w, h in TABLE_SIZES:
        d = sl.data_of(lname, w, h)
        want, pil_src = sl.oracle_std(d).rgb, pillow(d)
        for k, script in enumerate(SCRIPTS):
            case = (w, h, script)
            tw = table_twin(lname, w, h, k)
            plan, rs, dhts = jw.parse_script(script), scan_restarts(k), scan_dhts(tw)
            assert len(dhts) == len(plan) and all(len(t) == 2 * len(cs) for t, cs in zip(dhts, plan)), case
            s = mjx.ParsedScan(tw)
            try:
                dd = s.desc
                assert dd.n_parts == len(plan), case
                for j, cs in enumerate(plan):
                    p = dd.parts[j]
                    units = scan_units(lname, w, h, cs)
                    if [p.comp[q] for q in range(p.ncomp)] != cs or p.restart_interval != rs[j]:
                        bad.append(case + (j, "part", p.restart_interval))
                    if p.n_restart != (-(-units // rs[j]) - 1 if rs[j] else 0):
                        bad.append(case + (j, "restart offsets", p.n_restart, units))
                    for q in range(len(cs)):
                        for cls, tab in ((0, p.dc[q]), (1, p.ac[q])):
                            bits, vals = dhts[j][(cls, q)]
                            if list(tab.bits) != bits or list(tab.vals)[:len(vals)] != vals:
                                bad.append(case + (j, q, cls, "table"))
                if s.validate() != mjx.OK:
                    bad.append(case + ("validate", s.validate()))
            finally:
                s.close()
            if not np.array_equal(oracle_ms(tw).rgb, want):
                bad.append(case + ("oracle",))
            if not same_pillow(pillow(tw), pil_src):
                bad.append(case + ("pillow",))
    assert bad == [], bad


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_every_script_every_layout(mjx, gpu_ctx):
    """All 12 scripts x 64 layouts at 333 x 217, in mixed batches of 7-picture chunks, at scales 1, 2, 4 and 8: status OK and the
    GPU picture of the interleaved source bit for bit.  At scale 1 with keep_coefs (every picture gathered), T0 equals the oracle's
    ext_multiscan decode of the twin."""
    w, h = 333, 217
    cases = [(n, s, twins(n, w, h)[k]) for k, s in enumerate(SCRIPTS) for n in sl.NAMES]
    srcs = [sl.data_of(n, w, h) for n in sl.NAMES]
    bad = []
    for scale, keep in ((1, True), (1, False), (2, False), (4, False), (8, False)):
        want = dict(zip(sl.NAMES, sl.gpu_pictures(mjx, gpu_ctx, srcs, scale)))
        b, scans = sl.decode_batch(mjx, gpu_ctx, [c[2] for c in cases], scale=scale, keep_coefs=keep, chunk_images=7)
        try:
            for i, (n, s, tw) in enumerate(cases):
                if not isinstance(want[n], np.ndarray):
                    bad.append((n, scale, "source", want[n]))
                elif b.status(i) != mjx.OK:
                    bad.append((n, s, scale, "status", b.status(i)))
                elif not sl.same(b.rgb(i), want[n]):
                    bad.append((n, s, scale, keep, "rgb"))
                elif keep and not np.array_equal(b.coefs(i), orc_mod.interleave(oracle_ms(tw))):
                    bad.append((n, s, "T0"))
        finally:
            sl.close_all(b, scans)
    assert bad == [], bad


@pytest.mark.gpu
def test_pair_scans_take_the_direct_path_where_planar_ok_admits_them(mjx, gpu_ctx, tmp_path):
    """Each twin of PAIR_LAYOUTS at every twin size alone, at scales 1 and 8 (k_dc_color reads the DC values through the same slot
    rule as stage B): stage B reads the scans directly exactly where planar_direct says so, gathers everywhere else, and the
    picture is the interleaved source's bit for bit.  With MJX_PLANAR_DIRECT=0 every twin is gathered, alone and in one mixed
    batch, and the bytes are the same."""
    keys = [(n, w, h) for n in PAIR_LAYOUTS for w, h in sl.TWIN_SIZES]
    cases = [(n, w, h, s, twins(n, w, h)[k]) for n, w, h in keys for k, s in enumerate(SCRIPTS)]
    scales = (1, 8)
    bad, npair = [], 0
    want = {s: dict(zip(keys, sl.gpu_pictures(mjx, gpu_ctx, [sl.data_of(*key) for key in keys], s))) for s in scales}
    for scale in scales:
        for n, w, h, s, tw in cases:
            b, scans = sl.decode_batch(mjx, gpu_ctx, [tw], scale=scale)
            try:
                g = b.rgb(0) if b.status(0) == mjx.OK else None
                direct = g is not None and not sl.coefs_expand(mjx, b, 0)
            finally:
                sl.close_all(b, scans)
            npair += direct and " " in s
            if direct != planar_direct(n, w, s, scale):
                bad.append((n, w, h, s, scale, "direct path taken" if direct else "gather taken"))
            if not sl.same(g, want[scale][(n, w, h)]):
                bad.append((n, w, h, s, scale, "alone", "direct" if direct else "gather"))
    out, status, _, expands = sl.run_child(tmp_path, "gather", [c[-1] for c in cases], scales, {"MJX_PLANAR_DIRECT": "0"},
                                           single=True)
    for scale in scales:
        for i, (n, w, h, s, _) in enumerate(cases):
            for tag in ("all", "one"):
                key = "%d_%d_%s" % (i, scale, tag)
                if not sl.same(out.get(key), want[scale][(n, w, h)]):
                    bad.append((n, w, h, s, scale, "MJX_PLANAR_DIRECT=0", tag, status[key]))
            if not expands.get("%d_%d_one" % (i, scale)):
                bad.append((n, w, h, s, scale, "not gathered with MJX_PLANAR_DIRECT=0"))
    assert bad == [], bad
    assert npair >= 50, npair                   # (60 twins with a pair scan read directly)


@pytest.mark.gpu
def test_tables_between_scans_through_every_front_door(mjx, gpu_ctx):
    """Per-scan Huffman tables and restart intervals with COM / APP1 between the scans, and the DQT cases (a) to (c), through
    Batch (with keep_coefs: T0 as the oracle's), mjx_decode_batch (host and device de-stuffing) and the pool: status OK and the
    GPU picture of the interleaved source bit for bit."""
    w, h = 333, 217
    cases = []
    for n in TABLE_LAYOUTS:
        d = sl.data_of(n, w, h)
        cases += [("%s %s per-scan tables" % (n, s), d, table_twin(n, w, h, k)) for k, s in enumerate(SCRIPTS)]
        for dqt in DQT_CASES:
            src, tws = dqt_twins(n, w, h, dqt)
            cases += [("%s %s dqt %s" % (n, s, dqt), src, tw) for s, tw in zip(dqt_scripts(dqt), tws)]
    srcs = list(dict.fromkeys(c[1] for c in cases))
    want = dict(zip(srcs, sl.gpu_pictures(mjx, gpu_ctx, srcs, 1)))
    datas = [c[2] for c in cases]
    bad = []
    for keep in (True, False):
        b, scans = sl.decode_batch(mjx, gpu_ctx, datas, keep_coefs=keep, chunk_images=5)
        try:
            for i, (cn, src, tw) in enumerate(cases):
                if b.status(i) != mjx.OK:
                    bad.append((cn, "Batch", keep, b.status(i)))
                elif not sl.same(b.rgb(i), want[src]):
                    bad.append((cn, "Batch", keep, "rgb"))
                elif keep and not np.array_equal(b.coefs(i), orc_mod.interleave(oracle_ms(tw))):
                    bad.append((cn, "T0"))
        finally:
            sl.close_all(b, scans)
    for dd in (False, True):
        b, st = mjx.decode_batch(gpu_ctx, datas, device_destuff=dd)
        try:
            bad += [(cn, "mjx_decode_batch", dd, st[i]) for i, (cn, src, _) in enumerate(cases)
                    if st[i] != mjx.OK or not sl.same(b.rgb(i), want[src])]
        finally:
            b.close()
    pool = mjx.Pool([0])
    try:
        r = pool.decode_batch(datas)
        try:
            bad += [(cn, "pool", r.status[i]) for i, (cn, src, _) in enumerate(cases)
                    if r.status[i] != mjx.OK or not sl.same(r.rgb(i), want[src])]
        finally:
            r.close()
    finally:
        pool.close()
    assert bad == [], bad
