"""TEST INFRASTRUCTURE ONLY: torch-CPU stand-ins for the GRU decoder cell (asr_gru_cell_*) and for the decoder loops run
around it (asr_att_decoder_{fwd,bwd,infer,beam}_gru), layered over _cpu_ops.install so that the host logic of
AttentionSeq2Seq(decoder_type='gru') runs in the `-m "not gpu"` suite.  Each stand-in computes in float64 what its kernel
computes (the same split of the backward: dpre = dr | du | dp, d_in = dpre W3^T, the carried dh without d_in's h-columns)
and is the step-by-step statement the native loops are held against on the GPU.  A loop dict without a 'gru' block goes
to the stand-in _cpu_ops (or _cpu_ops_att_beam) has for it, untouched."""
import torch

import _cpu_ops
import _cpu_ops_att_beam

CALLS = dict(fwd=0, bwd=0, infer=0, beam=0)      # GRU loop calls since import (a test that must see none reads it)


def _gru_cell_prep(W_g, b_g, W_c, b_c):
    Din, U = W_c.shape
    W3 = torch.zeros((Din + 1, 3 * U), dtype=torch.float32)
    W3[:Din, :2 * U] = W_g
    W3[:Din - U, 2 * U:] = W_c[:Din - U]
    W3[Din, :2 * U] = b_g
    W3[Din, 2 * U:] = b_c
    return W3


def _gru_cell_gemm_ok(B, Din, U, ldx=None):
    ldx = Din if ldx is None else ldx
    return 1 <= B <= 32 and U >= 16 and U % 16 == 0 and Din > U and Din % 64 == 0 and ldx >= Din and ldx % 4 == 0


def _gru_cell_fwd(x, W3, W_c, h_prev, live, out_mask=None, fused=False, h_also=None, cell_out_also=None, out=None):
    B, Din = x.shape
    U = W_c.shape[1]
    if fused:
        assert _gru_cell_gemm_ok(B, Din, U, x.stride(0))
    x64, hp = x.double(), h_prev.double()
    pre = x64 @ W3[:Din].double() + W3[Din].double()
    r, u = torch.sigmoid(pre[:, :U]), torch.sigmoid(pre[:, U:2 * U])
    rh = r * hp
    c = torch.tanh(pre[:, 2 * U:] + rh @ W_c[Din - U:].double())
    hn = u * hp + (1 - u) * c
    lv = (live > 0).double().unsqueeze(1)
    ho = lv * hn + (1 - lv) * hp
    co = hn * out_mask.double() if out_mask is not None else hn
    gates, h_out, cell_out = out if out is not None else (torch.zeros(B, 4 * U), torch.zeros(B, U), torch.zeros(B, U))
    gates.copy_(torch.cat([r, u, c, rh], 1).float())
    h_out.copy_(ho.float())
    cell_out.copy_(co.float())
    if h_also is not None:
        h_also.copy_(ho.float())
    if cell_out_also is not None:
        cell_out_also.copy_(co.float())
    return gates, h_out, cell_out


def _gru_cell_bwd(dcell, dh_c, gates, h_prev, W3, W_c, live, out_mask=None, dh_c2=None):
    B, U = dcell.shape
    Din = W_c.shape[0]
    g = gates.double()
    r, u, c = g[:, :U], g[:, U:2 * U], g[:, 2 * U:3 * U]
    hp = h_prev.double()
    dhc = dh_c.double() + (dh_c2.double() if dh_c2 is not None else 0.0)
    lv = (live > 0).double().unsqueeze(1)
    dhn = (dcell.double() * out_mask.double() if out_mask is not None else dcell.double()) + lv * dhc
    dc, du = dhn * (1 - u), dhn * (hp - c)
    dp = dc * (1 - c * c)
    d_rh = dp @ W_c[Din - U:].double().t()
    dpre = torch.cat([d_rh * hp * r * (1 - r), du * u * (1 - u), dp], 1)
    d_in = dpre @ W3[:Din].double().t()
    carry = (1 - lv) * dhc + dhn * u + d_rh * r
    return dpre.float(), carry.float(), d_in.float()


def _attend(a, k, qz, nxt):
    C = _cpu_ops
    U, Em, E2, T = a['U'], a['Em'], a['E2'], a['T']
    if a['carry_alpha']:
        energy = C._att_loc_energy_fwd(a['alpha_all'][k - 1] if k > 0 else a['alpha_zero'], a['filt'], a['wfil'],
                                       a.get('keys'), qz, a['v'], T)
    else:
        energy = C._att_energy_fwd(a.get('keys'), qz, a.get('v'), T, a['att_mode'])
    sn = a.get('snorm_all')
    C._att_softmax_ctx_fwd(energy, a['seq_len'], a['sharpening'], a['enc'], alpha_out=a['alpha_all'][k],
                           sigmoid_norm=sn[k] if sn is not None else None,
                           ctx_also=(a['av_in'][k, :, U:], nxt[:, Em:Em + E2] if nxt is not None else None))


def _gru_fwd_step(a, W3, k, ks, nxt):
    """The forward step of the loops: cell (scatter targets as the kernels'), query FC, attention."""
    C = _cpu_ops
    U, Em, E2 = a['U'], a['Em'], a['E2']
    g = a['gru']
    dmask = a['dmask'][k] if a.get('dmask') is not None else None
    gates, h_new, cell_out = _gru_cell_fwd(a['dec_in'][k], W3, g['W_c'], a['h_all'][k], a['live'][k], out_mask=dmask,
                                           h_also=nxt[:, Em + E2:] if nxt is not None else None,
                                           cell_out_also=a['av_in'][k, :, :U])
    a['gates_all'][ks].copy_(gates)
    a['h_all'][k + 1].copy_(h_new)
    qz = C._gemm(cell_out, a['W_q'], bias=a.get('b_q')) if a['has_query_fc'] else cell_out
    a['qz_all'][ks].copy_(qz)
    _attend(a, k, qz, nxt)


def _image(a):
    g = a['gru']
    W3 = _gru_cell_prep(g['W_g'], g['b_g'], g['W_c'], g['b_c'])
    g['W3'] = W3
    return W3


def _att_decoder_fwd(a):
    if a.get('gru') is None:
        return _cpu_ops._att_decoder_fwd(a)
    CALLS['fwd'] += 1
    W3 = _image(a)
    To = a['To']
    for k in range(To):
        _gru_fwd_step(a, W3, k, k, a['dec_in'][k + 1] if k + 1 < To else None)


def _att_decoder_bwd(a):
    """asr_att_decoder_bwd_gru, step for step (the attention part as _cpu_ops._att_decoder_bwd)."""
    if a.get('gru') is None:
        return _cpu_ops._att_decoder_bwd(a)
    CALLS['bwd'] += 1
    C = _cpu_ops
    W3 = _image(a)
    To, B, U, Em, E2 = a['To'], a['B'], a['U'], a['Em'], a['E2']
    dh_carry = torch.zeros(B, U)
    dh2 = None
    dctx_in = torch.zeros(B, E2)
    dalpha_next = None
    sn = a.get('snorm_all')
    for k in range(To - 1, -1, -1):
        dctx = a['dctx_all'][k]
        torch.add(a['dav_ctx'][k], dctx_in, out=dctx)
        denergy = C._att_softmax_ctx_bwd(dctx, a['alpha_all'][k], a['seq_len'], a['sharpening'], a['enc'], None,
                                         sigmoid_norm=sn[k] if sn is not None else None, dalpha_extra=dalpha_next)
        dv_out = a['dv_all'][k] if a.get('dv_all') is not None else None
        if a['carry_alpha']:
            dqz, _, dalpha_next = C._att_loc_energy_bwd(
                denergy, a['alpha_all'][k - 1] if k > 0 else a['alpha_zero'], a['filt'], a['wfil'], a.get('keys'),
                a['qz_all'][k], a['v'], a['dwfil_rows'], a['dfilt_rows'], accumulate=(k != To - 1),
                dkeys=a.get('dkeys'), dqz_out=a['dqz_all'][k], dv_out=dv_out)
        else:
            dqz, _ = C._att_energy_bwd(denergy, a.get('keys'), a['qz_all'][k], a.get('v'), a['att_mode'],
                                       dkeys=a.get('dkeys'), want_dv=a['att_mode'] == 0, dqz_out=a['dqz_all'][k],
                                       dv_out=dv_out)
        dcell = a['dav_cell'][k]
        if a['has_query_fc']:
            C._gemm(dqz, a['W_q'], transB=True, out=dcell, accumulate=True)
        else:
            dcell += dqz
        dmask = a['dmask'][k] if a.get('dmask') is not None else None
        dpre, dh_carry, d_in = _gru_cell_bwd(dcell, dh_carry, a['gates_all'][k], a['h_all'][k], W3, a['gru']['W_c'],
                                             a['live'][k], out_mask=dmask, dh_c2=dh2)
        a['dpre_all'][k].copy_(dpre)
        a['d_in_all'][k].copy_(d_in)
        dctx_in = d_in[:, Em:Em + E2]
        dh2 = d_in[:, Em + E2:]
    a['dh0'].copy_(dh_carry + dh2)


def _att_decoder_infer(a, W_av, W_out, b_out, embedding, eos, n_live, check_every=8):
    if a.get('gru') is None:
        return _cpu_ops._att_decoder_infer(a, W_av, W_out, b_out, embedding, eos, n_live, check_every=check_every)
    CALLS['infer'] += 1
    C = _cpu_ops
    W3 = _image(a)
    To, B, U, Em, E2 = a['To'], a['B'], a['U'], a['Em'], a['E2']
    dec_in, av_in, live = a['dec_in'], a['av_in'], a['live']
    C2 = W_out.shape[1]
    out = dict(ids=torch.zeros((To, B), dtype=torch.int32), logits=torch.zeros((To, B, C2)), av=torch.zeros((To, B, U)),
               live=live, live_count=torch.zeros((To + 1,), dtype=torch.int32))
    out['live_count'][0] = int(n_live)
    issued = To
    for k in range(To):
        if check_every and k > 0 and k % check_every == 0 and int(out['live_count'][k]) == 0:
            issued = k
            break
        nxt = dec_in[k + 1] if k + 1 < To else None
        _gru_fwd_step(a, W3, k, 0, nxt)
        av = C._tanh_fwd(C._gemm(av_in[k], W_av))
        lg = C._gemm(av, W_out, bias=b_out)
        out['av'][k].copy_(av)
        out['logits'][k].copy_(lg)
        ids = C._argmax_rows(lg)
        lv = live[k]
        out['ids'][k].copy_((ids.float() * lv).to(torch.int32))
        live[k + 1].copy_(lv * (ids != int(eos)).float())
        out['live_count'][k + 1] = int(live[k + 1].sum())
        if nxt is not None:
            nxt[:, :Em].copy_(C._embedding_gather(embedding, ids))
            nxt[:, Em:Em + E2].mul_(lv.unsqueeze(1))
    out['steps_issued'] = issued
    return out


def _att_decoder_beam(a, *args, **kw):
    """The beam loop of _cpu_ops_att_beam with the LSTM cell's two stand-ins swapped for the GRU step for the time of the
    call (its selection / re-ordering / back-trace are the cell's business as little as the native loop's are)."""
    if a.get('gru') is None:
        return _cpu_ops_att_beam._att_decoder_beam(a, *args, **kw)
    CALLS['beam'] += 1
    W3 = _image(a)
    g = a['gru']
    C = _cpu_ops
    real_gemm, real_cell = C._gemm, C._lstm_cell_fwd
    marker = object()

    def gemm(A_, B_, *p, **k):
        if B_ is marker:                   # the cell-input product: nothing to do, the GRU step takes dec_in itself
            return A_
        return real_gemm(A_, B_, *p, **k)

    def cell(pre, c_prev, h_prev, peep, live, fb, clip, out_mask=None, want_cell_out=False, h_also=None, cell_out_also=None):
        gates, h_new, cell_out = _gru_cell_fwd(pre, W3, g['W_c'], h_prev, live, out_mask=out_mask, h_also=h_also,
                                               cell_out_also=cell_out_also)
        return gates, torch.zeros_like(h_new), torch.zeros_like(h_new), h_new, h_new, cell_out
    a = dict(a, W_cell=marker, b_cell=None)
    C._gemm, C._lstm_cell_fwd = gemm, cell
    try:
        return _cpu_ops_att_beam._att_decoder_beam(a, *args, **kw)
    finally:
        C._gemm, C._lstm_cell_fwd = real_gemm, real_cell


def _counts():
    return dict(fwd_fused=0, fwd_general=0, bwd=0)


STAND_INS = dict(gru_cell_prep=_gru_cell_prep, gru_cell_gemm_ok=_gru_cell_gemm_ok, gru_cell_fwd=_gru_cell_fwd,
                 gru_cell_bwd=_gru_cell_bwd, att_decoder_fwd=_att_decoder_fwd, att_decoder_bwd=_att_decoder_bwd,
                 att_decoder_infer=_att_decoder_infer, att_decoder_beam=_att_decoder_beam)


def install(monkeypatch):
    ops = _cpu_ops_att_beam.install(monkeypatch)
    for name, fn in STAND_INS.items():
        assert hasattr(ops, name), name
        monkeypatch.setattr(ops, name, fn)
    return ops
