#!/usr/bin/env python
"""Print reference / hypothesis pairs of a trained CTC model on the TIMIT test set -- the recipe of
examples/timit/visualization/decode_ctc.py (restore a run directory, decode, print `Ref:` / `Hyp:` per utterance).

    python examples/timit/visualization/decode_ctc.py <model_path> [--epoch E] [--beam_width W] [--max_utt N]"""
import argparse
import sys
from os.path import abspath, dirname, isfile, join

import numpy as np
import yaml

ROOT = dirname(dirname(dirname(dirname(abspath(__file__)))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from examples.timit.data.load_dataset_ctc import Dataset                                                     # noqa: E402
from examples.timit.metrics.mapping_files import write_mapping_files                                         # noqa: E402
from examples.timit.training.train_ctc import build_model                                                    # noqa: E402
from tensorflow_end2end_speech_recognition_amd.utils.io.labels.character import Idx2char                     # noqa: E402
from tensorflow_end2end_speech_recognition_amd.utils.io.labels.phone import Idx2phone                        # noqa: E402
from tensorflow_end2end_speech_recognition_amd.utils.io.labels.sparsetensor import sparsetensor2list         # noqa: E402
from tensorflow_end2end_speech_recognition_amd.utils.training.checkpoint import Saver, get_checkpoint_state  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('model_path')
    ap.add_argument('--epoch', type=int, default=-1)
    ap.add_argument('--beam_width', type=int, default=20)
    ap.add_argument('--max_utt', type=int, default=None)
    ap.add_argument('--device', default=None)
    args = ap.parse_args(argv)
    with open(join(args.model_path, 'config.yml'), 'r') as f:
        params = yaml.safe_load(f)['param']
    if args.device:
        params['device'] = args.device
    model = build_model(params)
    ckpt = get_checkpoint_state(args.model_path)
    if ckpt is None:
        raise ValueError('There are not any checkpoints.')
    path = ckpt.model_checkpoint_path if args.epoch == -1 else join(args.model_path, 'model.ckpt-' + str(args.epoch))
    Saver().restore(model, path)
    map_dir = params.get('map_dir') or join(args.model_path, 'mapping_files')
    if not isfile(join(map_dir, 'phone2phone.txt')):
        write_mapping_files(map_dir)
    is_char = 'char' in params['label_type']
    if params['label_type'] == 'character_capital_divide':
        to_str = Idx2char(join(map_dir, 'character_capital_divide.txt'), capital_divide=True, space_mark='_')
    elif is_char:
        to_str = Idx2char(join(map_dir, 'character.txt'))
    else:
        to_str = Idx2phone(join(map_dir, params['label_type'] + '.txt'))
    test_data = Dataset(data_type='test', label_type=params['label_type'] if is_char else 'phone39', batch_size=1,
                        splice=params['splice'], num_stack=params['num_stack'], num_skip=params['num_skip'],
                        sort_utt=False, dataset_root=params.get('dataset_root'))
    pairs = []
    for (inputs, labels_true, inputs_seq_len, input_names), is_new_epoch in test_data:
        B = inputs[0].shape[0]
        _, logits = model.compute_loss(inputs[0], np.zeros((B, 1), dtype=np.int64), inputs_seq_len[0], keep_prob=1.0,
                                       is_training=False)
        hyps = sparsetensor2list(model.decoder(logits, model.output_seq_len(inputs_seq_len[0]),
                                               beam_width=args.beam_width), B)
        for b in range(B):
            ref, hyp = labels_true[0][b][0], to_str(np.asarray(hyps[b], dtype=np.int64))
            pairs.append((str(input_names[0][b]), ref, hyp))
            print('----- wav: %s -----' % input_names[0][b])
            print('Ref: %s' % ref)
            print('Hyp: %s' % hyp)
        if is_new_epoch or (args.max_utt is not None and len(pairs) >= args.max_utt):
            break
    return pairs


if __name__ == '__main__':
    main()
