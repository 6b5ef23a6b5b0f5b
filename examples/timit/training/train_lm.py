#!/usr/bin/env python
"""Train an RNN language model on the label sequences of the TIMIT attention dataset.

    python examples/timit/training/train_lm.py <config.yml> <model_save_path>

EXTENSION (the reference has no language model recipe: its models/lm classes raise NotImplementedError).  Flow as
train_attention.py (shared loop in _common.py): the dataset is the attention recipe's -- <SOS> y <EOS> targets and their
lengths; the features are ignored --, the monitored "label error rate" is the token error rate of the teacher-forced
argmax, and the epoch metric the dev perplexity normalised to (0, 1] as 1 - 1 / perplexity (lower is better, as the loop
expects).  The run directory is <model_save_path>/lm/<label_type>/<name>; eval_attention.py --lm_path reads it."""
import sys
from os.path import abspath, dirname, isfile, join

import numpy as np
import yaml

ROOT = dirname(dirname(dirname(dirname(abspath(__file__)))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from examples.timit.data.load_dataset_attention import Dataset                                              # noqa: E402
from examples.timit.metrics.mapping_files import write_mapping_files                                        # noqa: E402
from examples.timit.training._common import NUM_CLASSES, new_run_directory, run_with_log, training_loop      # noqa: E402
from examples.timit.training.train_attention import make_datasets                                           # noqa: E402
from tensorflow_end2end_speech_recognition_amd.models.lm.base import RNNLM                                  # noqa: E402
from tensorflow_end2end_speech_recognition_amd.utils.training.checkpoint import Saver, get_checkpoint_state  # noqa: E402


def model_kwargs(params):
    n = params['num_classes']
    return dict(num_classes=n + 2, embedding_dim=params['embedding_dim'], num_units=params['num_units'],
                num_layers=params['num_layers'], sos_index=n, eos_index=n + 1, parameter_init=params['weight_init'],
                clip_grad_norm=params['clip_grad_norm'], clip_activation=params['clip_activation'],
                weight_decay=params['weight_decay'], device=params.get('device', 'cuda:0'))


def run_name(params):
    name = 'lstm' + str(params['num_units']) + '_' + str(params['num_layers']) + '_emb' + str(params['embedding_dim'])
    name += '_' + params['optimizer'] + '_lr' + str(params['learning_rate'])
    if params['dropout'] != 0:
        name += '_drop' + str(params['dropout'])
    if params['weight_decay'] != 0:
        name += 'wd' + str(params['weight_decay'])
    return name


def restore_lm(run_dir, epoch=-1, device=None):
    """The RNNLM of a run directory of this recipe, restored from its latest (or the given epoch's) checkpoint."""
    with open(join(run_dir, 'config.yml'), 'r') as f:
        params = yaml.safe_load(f)['param']
    if device:
        params['device'] = device
    params['num_classes'] = NUM_CLASSES[params['label_type']]
    model = RNNLM(**model_kwargs(params))
    ckpt = get_checkpoint_state(run_dir)
    if ckpt is None:
        raise ValueError('There are not any checkpoints.')
    Saver().restore(model, ckpt.model_checkpoint_path if epoch == -1 else join(run_dir, 'model.ckpt-' + str(epoch)))
    return model


def token_error_rate(logits, labels, labels_seq_len):
    """Share of scored positions whose teacher-forced argmax is not the next label."""
    pred = np.asarray(logits.argmax(dim=2).cpu())
    labels, lens = np.asarray(labels), np.asarray(labels_seq_len)
    live = np.arange(pred.shape[1])[None, :] < (lens - 1)[:, None]
    return float(((pred != labels[:, 1:pred.shape[1] + 1]) & live).sum()) / max(int(live.sum()), 1)


def do_train(model, params):
    map_dir = params.get('map_dir') or join(model.save_path, 'mapping_files')
    if not isfile(join(map_dir, 'phone2phone.txt')):
        write_mapping_files(map_dir)
    train_data, dev_data, test_data = make_datasets(Dataset, params, map_dir)
    keep = 1 - float(params['dropout'])
    dev_ppl = [None]                      # the perplexity of the last dev evaluation

    def train_step(data, learning_rate):
        _, labels, _, labels_seq_len, _ = data
        loss, _ = model.compute_loss(labels[0], labels_seq_len[0], keep)
        model.train(loss, optimizer=params['optimizer'], learning_rate=learning_rate)

    def monitor(data):
        _, labels, _, labels_seq_len, _ = data
        loss, logits = model.compute_loss(labels[0], labels_seq_len[0], 1.0, is_training=False)
        return float(loss), token_error_rate(logits, labels[0], labels_seq_len[0])

    def evaluate(is_test):
        if is_test:                      # the test set is labelled with 39 phones, another vocabulary: it is not scored;
            if dev_ppl[0] is None:       # the loop asks behind a new best dev value and gets that value back
                raise RuntimeError('train_lm: no dev evaluation precedes the test evaluation')
            return 1.0 - 1.0 / dev_ppl[0]
        nll = tokens = 0.0
        for data, is_new_epoch in dev_data:
            _, labels, _, labels_seq_len, _ = data
            model.compute_loss(labels[0], labels_seq_len[0], 1.0, is_training=False)
            n = float((np.asarray(labels_seq_len[0]) - 1).sum())
            nll += float(model.sequence_loss) * n
            tokens += n
            if is_new_epoch:
                break
        dev_ppl[0] = float(np.exp(nll / max(tokens, 1.0)))
        print('  perplexity: %f' % dev_ppl[0])
        return 1.0 - 1.0 / dev_ppl[0]

    return training_loop(model, params, train_data, dev_data, train_step, monitor, evaluate, '1 - 1/PPL')


def main(config_path, model_save_path, log_to_file=True):
    with open(config_path, 'r') as f:
        params = yaml.safe_load(f)['param']
    if params['label_type'] not in NUM_CLASSES:
        raise TypeError
    params['num_classes'] = NUM_CLASSES[params['label_type']]
    model = RNNLM(**model_kwargs(params))
    model.name = run_name(params)
    model.save_path = new_run_directory(join(model_save_path, 'lm', params['label_type'], model.name), config_path)
    result = run_with_log(lambda: do_train(model, params), model.save_path, log_to_file)
    result.update(save_path=model.save_path, model=model)
    return result


if __name__ == '__main__':
    args = sys.argv
    if len(args) != 3:
        raise ValueError('Length of args should be 3.')
    main(config_path=args[1], model_save_path=args[2])
