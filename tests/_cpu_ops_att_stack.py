"""TEST INFRASTRUCTURE ONLY: torch-CPU stand-ins for the decoder loops with a multi-layer LSTM decoder
(asr_att_decoder_{fwd,bwd,infer,beam}_stack, asr_att_stack_reorder, asr_att_stack_bwd_step), layered over
_cpu_ops_att_gru.install so that the host logic of AttentionSeq2Seq(decoder_num_layers > 1) runs in the `-m "not gpu"`
suite.  Each stand-in computes in float64 what its kernels compute, in the native loops' order (layer 0's masked output into
the input row of layer 1, the upper layers' cells, the top layer's output into av_in / the query; backwards the top layer's
cell, then per lower layer dx = dpre W^T of the layer above and its own cell), and is the step-by-step statement the native
loops are held against on the GPU.  A loop dict without a 'stack' block goes to the stand-in below it, untouched."""
import torch

import _cpu_ops
import _cpu_ops_att_beam
import _cpu_ops_att_gru

CALLS = dict(fwd=0, bwd=0, infer=0, beam=0)      # stack loop calls since import (a test that must see none reads it)


def _stack_fwd_step(a, k, ks, nxt_k):
    """Cells of forward step k: layer 0 (asr_att_decoder's), then the upper layers; returns the top layer's masked output.
    nxt_k: the row block index the next step reads (k + 1; the beam's 1), or None behind the last step."""
    C = _cpu_ops
    U, Em, E2 = a['U'], a['Em'], a['E2']
    ups = a['stack']['layers']
    live = a['live'].reshape(-1, a['B'])[k] if a['live'].dim() > 1 else a['live']
    nxt = a['dec_in'][nxt_k] if nxt_k is not None else None
    pre = C._gemm(a['dec_in'][k], a['W_cell'], bias=a['b_cell'])
    dmask = a['dmask'][k] if a.get('dmask') is not None else None
    gates, c_raw, c_new, h_new, _, _ = C._lstm_cell_fwd(
        pre, a['c_all'][k], a['h_all'][k], a.get('peep'), live, a['forget_bias'], a['cell_clip'], out_mask=dmask,
        want_cell_out=True, h_also=nxt[:, Em + E2:] if nxt is not None else None, cell_out_also=ups[0]['in'][k][:, :U])
    a['gates_all'][ks].copy_(gates)
    a['craw_all'][ks].copy_(c_raw)
    a['c_all'][k + 1 if nxt_k is None else nxt_k].copy_(c_new)
    a['h_all'][k + 1 if nxt_k is None else nxt_k].copy_(h_new)
    cell_out = None
    for i, u in enumerate(ups):
        top = i + 1 == len(ups)
        pre = C._gemm(u['in'][k], u['W'], bias=u['b'])
        mask = u['dmask'][k] if u.get('dmask') is not None else None
        gates, c_raw, c_new, h_new, _, cell_out = C._lstm_cell_fwd(
            pre, u['c'][k], u['h'][k], u.get('peep'), live, a['forget_bias'], a['cell_clip'], out_mask=mask,
            want_cell_out=True, h_also=u['in'][nxt_k][:, U:] if nxt_k is not None else None,
            cell_out_also=a['av_in'][k, :, :U] if top else ups[i + 1]['in'][k][:, :U])
        u['gates'][ks].copy_(gates)
        u['craw'][ks].copy_(c_raw)
        u['c'][k + 1 if nxt_k is None else nxt_k].copy_(c_new)
        u['h'][k + 1 if nxt_k is None else nxt_k].copy_(h_new)
    return cell_out


def _fwd_step(a, k, ks, nxt_k):
    C = _cpu_ops
    cell_out = _stack_fwd_step(a, k, ks, nxt_k)
    qz = C._gemm(cell_out, a['W_q'], bias=a.get('b_q')) if a['has_query_fc'] else cell_out
    a['qz_all'][ks].copy_(qz)
    _cpu_ops_att_gru._attend(a, k, qz, a['dec_in'][nxt_k] if nxt_k is not None else None)


def _att_decoder_fwd(a):
    if a.get('stack') is None:
        return _cpu_ops_att_gru._att_decoder_fwd(a)
    CALLS['fwd'] += 1
    To = a['To']
    for k in range(To):
        _fwd_step(a, k, k, k + 1 if k + 1 < To else None)


def _att_stack_bwd_step(dpre_up, W_up, dc_next, dh_next, gates, c_raw, c_prev, live, peep=None, use_mask=None, dh_next2=None,
                        fused=True, want_dpeep=None):
    """asr_att_stack_bwd_step: dx = dpre_up W_up^T; the cell backward on dx[:, :U] * use_mask; d_hin_up = dx[:, U:]."""
    C = _cpu_ops
    B, U = dc_next.shape
    dx = dpre_up.double() @ W_up.double().t()
    g = dx[:, :U] * (use_mask.double() if use_mask is not None else 1.0)
    dhn = dh_next.double() + (dh_next2.double() if dh_next2 is not None else 0.0)
    want = (peep is not None) if want_dpeep is None else want_dpeep
    dpre, dc_prev, carry, dpeep = C._lstm_cell_bwd(g.float(), dc_next, dhn.float(), gates, c_raw, c_prev, peep, live,
                                                   want_dpeep=want)
    return dpre, dc_prev, carry, dx[:, U:].float(), dpeep.reshape(B, 3 * U) if dpeep is not None else None


def _att_decoder_bwd(a):
    """asr_att_decoder_bwd_stack, step for step (the attention part as _cpu_ops._att_decoder_bwd)."""
    if a.get('stack') is None:
        return _cpu_ops_att_gru._att_decoder_bwd(a)
    CALLS['bwd'] += 1
    C = _cpu_ops
    To, B, U, Em, E2 = a['To'], a['B'], a['U'], a['Em'], a['E2']
    ups = a['stack']['layers']
    L = len(ups) + 1
    dc = [torch.zeros(B, U) for _ in range(L)]
    dh = [torch.zeros(B, U) for _ in range(L)]       # carried dh, WITHOUT the h-columns of the next step's input gradient
    dh2 = [None] * L
    dctx_in = torch.zeros(B, E2)
    dalpha_next = None
    sn = a.get('snorm_all')

    def cell_bwd(l, k, g):
        """the cell backward of layer l at step k on g (gradient w.r.t. its masked output)"""
        lay = ups[l - 1] if l else None
        mask = (lay.get('dmask') if l else a.get('dmask'))
        dpeep_all = (lay.get('dpeep') if l else a.get('dpeep_all'))
        if mask is not None:
            g = C._apply_mask(g, mask[k])
        dhn = dh[l] + dh2[l] if dh2[l] is not None else dh[l]
        dpre, dc[l], dh[l], _ = C._lstm_cell_bwd(
            g, dc[l], dhn, (lay['gates'] if l else a['gates_all'])[k], (lay['craw'] if l else a['craw_all'])[k],
            (lay['c'] if l else a['c_all'])[k], lay.get('peep') if l else a.get('peep'), a['live'][k],
            want_dpeep=dpeep_all is not None, dpre_out=(lay['dpre'] if l else a['dpre_all'])[k],
            dpeep_out=dpeep_all[k] if dpeep_all is not None else None)
        return dpre

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
        g = a['dav_cell'][k]
        if a['has_query_fc']:
            C._gemm(dqz, a['W_q'], transB=True, out=g, accumulate=True)
        else:
            g += dqz
        for l in range(L - 1, 0, -1):                # the top layer's cell, then down: dx of layer l, the cell of layer l-1
            dpre = cell_bwd(l, k, g)
            dx = C._gemm(dpre, ups[l - 1]['W'], transB=True)
            ups[l - 1]['d_hin'][k].copy_(dx[:, U:])
            dh2[l] = dx[:, U:]
            g = dx[:, :U].contiguous()
        dpre = cell_bwd(0, k, g)
        d_in = C._gemm(dpre, a['W_cell'], transB=True, out=a['d_in_all'][k])
        dctx_in = d_in[:, Em:Em + E2]
        dh2[0] = d_in[:, Em + E2:]
    a['dc0'].copy_(dc[0])
    a['dh0'].copy_(dh[0] + dh2[0])
    for l in range(1, L):
        ups[l - 1]['dc0'].copy_(dc[l])
        ups[l - 1]['dh0'].copy_(dh[l] + dh2[l])


def _att_decoder_infer(a, W_av, W_out, b_out, embedding, eos, n_live, check_every=8):
    if a.get('stack') is None:
        return _cpu_ops_att_gru._att_decoder_infer(a, W_av, W_out, b_out, embedding, eos, n_live, check_every=check_every)
    CALLS['infer'] += 1
    C = _cpu_ops
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
        if nxt is None:                    # (the last step has no next input row: the state rows To exist all the same)
            _fwd_step(a, k, 0, None)
        else:
            _fwd_step(a, k, 0, k + 1)
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


def _att_stack_reorder(parent, c, h, in_):
    """asr_att_stack_reorder: block 1 -> block 0 by parent, every upper layer."""
    pr = _cpu_ops_att_beam._rows(parent)
    U = c[0].shape[2]
    for ci, hi, xi in zip(c, h, in_):
        ci[0].copy_(ci[1][pr])
        hi[0].copy_(hi[1][pr])
        xi[0][:, U:].copy_(xi[1][pr][:, U:])


def _att_decoder_beam(a, *args, **kw):
    """The beam loop of _cpu_ops_att_beam with the cell's two stand-ins swapped for the stacked step and the re-ordering
    extended to the upper layers for the time of the call (selection and back-trace are the cell's business as little as
    the native loop's are)."""
    if a.get('stack') is None:
        return _cpu_ops_att_gru._att_decoder_beam(a, *args, **kw)
    CALLS['beam'] += 1
    C, Bm = _cpu_ops, _cpu_ops_att_beam
    ups = a['stack']['layers']
    real_gemm, real_cell, real_reorder = C._gemm, C._lstm_cell_fwd, Bm._att_beam_reorder
    marker = object()
    inner = dict(a)

    def gemm(A_, B_, *p, **k):
        if B_ is marker:                   # layer 0's cell-input product: the stacked step below does it itself
            return A_
        return real_gemm(A_, B_, *p, **k)

    def cell(pre, c_prev, h_prev, peep, live, fb, clip, out_mask=None, want_cell_out=False, h_also=None, cell_out_also=None):
        C._gemm, C._lstm_cell_fwd = real_gemm, real_cell
        try:
            cell_out = _stack_fwd_step(inner, 0, 0, 1)
        finally:
            C._gemm, C._lstm_cell_fwd = gemm, cell
        return (a['gates_all'][0], a['craw_all'][0], a['c_all'][1].clone(), a['h_all'][1].clone(), a['h_all'][1].clone(),
                cell_out)

    def reorder(parent, *p):
        _att_stack_reorder(parent, [u['c'] for u in ups], [u['h'] for u in ups], [u['in'] for u in ups])
        return real_reorder(parent, *p)
    outer = dict(a, W_cell=marker, b_cell=None)
    C._gemm, C._lstm_cell_fwd, Bm._att_beam_reorder = gemm, cell, reorder
    try:
        return Bm._att_decoder_beam(outer, *args, **kw)
    finally:
        C._gemm, C._lstm_cell_fwd, Bm._att_beam_reorder = real_gemm, real_cell, real_reorder


def _att_stack_counts(device=0):
    return dict(fwd_image=0, fwd_two_launch=0, bwd_fused=0, bwd_generic=0)


def _att_stack_bwd_ok(B, U):
    return 1 <= B <= 32 and U >= 16 and U % 16 == 0


STAND_INS = dict(att_decoder_fwd=_att_decoder_fwd, att_decoder_bwd=_att_decoder_bwd, att_decoder_infer=_att_decoder_infer,
                 att_decoder_beam=_att_decoder_beam, att_stack_reorder=_att_stack_reorder,
                 att_stack_bwd_step=_att_stack_bwd_step, att_stack_counts=_att_stack_counts,
                 att_stack_bwd_ok=_att_stack_bwd_ok)


def install(monkeypatch):
    ops = _cpu_ops_att_gru.install(monkeypatch)
    for name, fn in STAND_INS.items():
        assert hasattr(ops, name), name
        monkeypatch.setattr(ops, name, fn)
    return ops
