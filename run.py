#!/usr/bin/env python
"""Command line front end of the MI355X GRU4Rec path.

It accepts the same flags, prints the same progress lines and uses the same exit codes as the reference's `run.py`, so
shell scripts and `paropt.py` (which scrapes the `PRIMARY METRIC:` line) keep working; the work itself goes through the
plugin class selected with `-g` (any module exposing `GRU4Rec`; default: the HIP implementation).
"""
import argparse
import importlib
import importlib.util
import os
import sys
import time
from collections import OrderedDict

KEY_COLUMNS = (          # (what it is, CLI attribute, default column, model parameter that overrides it)
    ('session IDs', 'session_key', 'SessionId'),
    ('item IDs', 'item_key', 'ItemId'),
    ('time', 'time_key', 'Time'),
)

# flag table: (short, long, argparse keywords)
OPTIONS = [
    ('-ps', '--parameter_string', dict(metavar='PARAM_STRING', help='hyper-parameters inline: name=value pairs separated by commas; list values use "/" (layers=100/100)')),
    ('-pf', '--parameter_file', dict(metavar='PARAM_PATH', help='python file that defines an OrderedDict called gru4rec_params')),
    ('-l', '--load_model', dict(action='store_true', help='PATH is a saved model: skip training')),
    ('-s', '--save_model', dict(metavar='MODEL_PATH', help='where to pickle the trained model (not saved by default)')),
    ('-t', '--test', dict(metavar='TEST_PATH', nargs='+', help='one or more test sets to evaluate on')),
    ('-m', '--measure', dict(metavar='AT', type=int, nargs='+', default=[20], help='cut-offs N for Recall@N / MRR@N (default 20)')),
    ('-e', '--eval_type', dict(metavar='EVAL_TYPE', choices=['standard', 'conservative', 'median', 'tiebreaking'], default='standard',
                               help='tie handling when ranking the target item (default standard)')),
    ('-ss', '--sample_store_size', dict(metavar='SS', type=int, default=10000000, help='number of pre-drawn negative samples kept on the device (default 10000000)')),
    (None, '--sample_store_on_cpu', dict(action='store_true', help='draw the negative samples with the reference\'s host sampler (NumPy stream) and upload them store by store, instead of sampling on the device')),
    ('-g', '--gru4rec_model', dict(metavar='GRFILE', default='gru4rec_amd.gru4rec', help='module that provides the GRU4Rec class (default gru4rec_amd.gru4rec)')),
    ('-ik', '--item_key', dict(metavar='IK', default='ItemId', help='item id column (default ItemId)')),
    ('-sk', '--session_key', dict(metavar='SK', default='SessionId', help='session id column (default SessionId)')),
    ('-tk', '--time_key', dict(metavar='TK', default='Time', help='timestamp column (default Time)')),
    ('-pm', '--primary_metric', dict(metavar='METRIC', choices=['recall', 'mrr'], default='recall', help='metric reported on the PRIMARY METRIC line (default recall)')),
    ('-lpm', '--log_primary_metric', dict(action='store_true', help='print the PRIMARY METRIC line after every evaluation')),
    (None, '--sparse_exact', dict(action='store_true', help='with --gpus N: keep the replicas bit-identical by exchanging every rank\'s per-occurrence gradient rows of the item tables every step (one RCCL all-gather) instead of reconciling GPU-local rows every sync_every steps.  REDUCE form: all ranks draw ONE stream of negatives, the gradient rows of a shared negative are summed over the ranks before the optimizer rule and every row is scaled by 1 / N -- the update of one batch of N x batch_size rows, except that a row meets only its own rank\'s in-batch negatives; for catalogues whose exchanged list fits the LDS')),
    (None, '--save_recs', dict(metavar='PATH', help='with -t (not in the reference): also write the top-k recommendation list, the target\'s rank and score of every test event to PATH as .npz (evaluation.recommend_gpu; several test sets: PATH gets the set\'s number in front of its extension)')),
    (None, '--recs_k', dict(metavar='K', type=int, default=20, help='list length of --save_recs (default 20)')),
    (None, '--gpus', dict(metavar='N', type=int, default=1, help='train on N GPUs of this node (not in the reference): one process per GPU, sessions sharded over '
                          'the ranks, dense GRU gradients all-reduced by RCCL every step, item rows GPU-local and reconciled every sync_every steps (4 at two ranks, 16 from three on) and at every epoch end; rank 0 saves / evaluates')),
]
# item-to-item neighbours (not in the reference): a table of their own, after training or loading
NEIGHBOR_OPTIONS = [
    (None, '--save_neighbors', dict(metavar='PATH', help='after training or loading (not in the reference): write every item\'s nearest neighbours in the model\'s output embedding to PATH as .npz -- item_ids, neighbor_ids, scores (GRU4Rec.item_neighbors)')),
    (None, '--neighbors_k', dict(metavar='K', type=int, default=20, help='neighbours per item of --save_neighbors (default 20)')),
    (None, '--neighbors_metric', dict(metavar='METRIC', choices=['cosine', 'dot'], default='cosine', help='similarity of --save_neighbors (default cosine)')),
]
# item groups (not in the reference): a table of their own as well
GROUP_OPTIONS = [
    (None, '--item_groups', dict(metavar='FILE', help='after training or loading (not in the reference): a TAB separated file of two columns, item id and group label, without a header; the groups are set on the model (GRU4Rec.set_item_groups: max_per_group / exclude_groups of the recommendation calls), so a model saved with -s carries them.  --save_recs is unaffected')),
]

# held-out log-likelihood (not in the reference): one more table
LOGLIK_OPTIONS = [
    (None, '--loglik', dict(action='store_true', help='with -t (not in the reference): also print the held-out negative log-likelihood and perplexity of the test set -- the mean of -log softmax(z / T)[next item] over its events (evaluation.loglik_gpu)')),
    (None, '--loglik_temperature', dict(metavar='T', type=float, default=1.0, help='temperature T of --loglik (default 1.0)')),
]

# audience selection (not in the reference): which sessions for this item?
AUDIENCE_OPTIONS = [
    (None, '--save_audience', dict(metavar='PATH', help='with -t (not in the reference): for every item of --audience_items the --audience_k test sessions most likely to continue with it -- the histories are the test sessions\' full sequences -- written to PATH as .npz: item_ids, session_ids (-1 behind a row\'s count), values, counts (GRU4Rec.audience_sessions; several test sets: PATH gets the set\'s number in front of its extension)')),
    (None, '--audience_items', dict(metavar='FILE', help='the items of --save_audience: a text file with one item id per line')),
    (None, '--audience_k', dict(metavar='K', type=int, default=100, help='sessions per item of --save_audience (default 100)')),
    (None, '--audience_by', dict(metavar='BY', choices=['score', 'logprob'], default='logprob', help='the value --save_audience ranks the sessions by: the item\'s score, or its log-probability under the session\'s next-item distribution (default logprob)')),
]


def build_parser():
    ap = argparse.ArgumentParser(description='Train a GRU4Rec model on an MI355X (or load one) and report Recall@N / MRR@N.')
    ap.add_argument('path', metavar='PATH', help='training data (.tsv / .txt with TAB separators, or a pickled DataFrame) -- or the model file when -l is given')
    for short, long_, kw in OPTIONS + NEIGHBOR_OPTIONS + GROUP_OPTIONS + LOGLIK_OPTIONS + AUDIENCE_OPTIONS:
        ap.add_argument(*([short, long_] if short else [long_]), **kw)
    return ap


def fail_missing_column(what, column, default, fname):
    print('ERROR. The column specified for {} "{}" is not in the data file ({})'.format(what, column, fname))
    print('The default column name is "{}", but you can specify otherwise by setting the `{}` parameter of the model.'.format(
        default, {'session IDs': 'session_key', 'item IDs': 'item_key', 'time': 'time_key'}[what]))
    sys.exit(1)


def read_events(fname, opts, model_cls=None):
    """Event table with the three key columns.  Item ids are kept as strings, session ids as int32.  Plugins that declare
    `accepts_categorical_items` get the table from the native multi-threaded parser (item ids as a categorical column)."""
    import pandas as pd
    wanted = [(what, getattr(opts, attr), default) for what, attr, default in KEY_COLUMNS]
    pickled = fname.endswith('.pickle')
    if pickled:
        import joblib
        print('Loading data from pickle file: {}'.format(fname))
        table = joblib.load(fname)
        present = set(table.columns)
    else:
        with open(fname, 'rt') as fh:
            present = set(fh.readline().rstrip('\r\n').split('\t'))
    for what, column, default in wanted:
        if column not in present:
            fail_missing_column(what, column, default, fname)
    if pickled:
        return table
    print('Loading data from TAB separated file: {}'.format(fname))
    if getattr(model_cls, 'accepts_categorical_items', False):
        from gru4rec_amd import eventio
        return eventio.read_events(fname, opts.session_key, opts.item_key, opts.time_key)
    cols = [c for _, c, _ in wanted]
    return pd.read_csv(fname, sep='\t', usecols=cols, dtype={opts.session_key: 'int32', opts.item_key: 'str'})


def hyper_parameters(opts):
    if opts.parameter_file:
        where = os.path.abspath(opts.parameter_file)
        spec = importlib.util.spec_from_file_location(os.path.splitext(os.path.basename(where))[0], where)
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
        print('Loaded parameters from file: {}'.format(where))
        return module.gru4rec_params
    return OrderedDict(item.split('=') for item in opts.parameter_string.split(','))


def set_item_groups(model, fname):
    """--item_groups: the (item id, group label) rows of a TAB separated file onto the model; items of the file the model does not
    know are dropped (a catalogue file usually lists more than the training data holds)."""
    import pandas as pd
    if not hasattr(model, 'set_item_groups'):
        print('ERROR. The model class {} does not support --item_groups'.format(type(model).__module__))
        sys.exit(1)
    table = pd.read_csv(fname, sep='\t', header=None, names=['item', 'group'], dtype=str, keep_default_na=False)
    known = table[table['item'].isin(model.itemidmap.index.astype(str))].drop_duplicates('item', keep='last')
    ids = dict(zip(model.itemidmap.index.astype(str), model.itemidmap.index))      # (a pickled table may hold ids that are not strings)
    model.set_item_groups({ids[i]: g for i, g in zip(known['item'], known['group'])})
    print('Item groups from {}: {} of {} items in {} groups'.format(fname, len(known), len(model.itemidmap), len(model.group_labels)))


def train(model_cls, opts):
    params = hyper_parameters(opts)
    print('Creating GRU4Rec model')
    model = model_cls()
    model.set_params(**params)
    rank, world = 0, 1
    if opts.gpus > 1 or os.environ.get('G4R_FORCE_STAGED'):
        # a rank of `run.py --gpus N` (spawned by main() below, or by torch.distributed.run): the communicator is created inside fit
        from gru4rec_amd import launch
        rank, world, local_rank = launch.layout()
        if world != opts.gpus:
            print('ERROR. WORLD_SIZE ({}) does not match --gpus ({})'.format(world, opts.gpus))
            sys.exit(1)
        if not hasattr(model, 'set_distributed'):
            print('ERROR. The model class {} does not support --gpus'.format(model_cls.__module__))
            sys.exit(1)
        model.device = local_rank
        model.sparse_exact = bool(opts.sparse_exact)
        model.set_distributed(rank, world, launch.unique_id(rank, world))
    print('Loading training data...')
    events = read_events(opts.path, opts, model_cls)
    if opts.sample_store_on_cpu:
        print('WARNING! The sample store is set to be on the CPU. This will make training significantly slower on the GPU.')
    print('Started training')
    started = time.time()
    model.fit(events, sample_store=opts.sample_store_size, store_type='cpu' if opts.sample_store_on_cpu else 'gpu')
    print('Total training time: {:.2f}s'.format(time.time() - started))
    if rank != 0:
        # replicas are identical after the last reconciliation: rank 0 alone saves and evaluates
        model.close()
        sys.exit(0)
    if world > 1:
        from gru4rec_amd import launch
        launch.cleanup(rank)
    if opts.item_groups:
        set_item_groups(model, opts.item_groups)
    if opts.save_model is not None:
        print('Saving trained model to: {}'.format(opts.save_model))
        model.savemodel(opts.save_model)
    return model


def evaluate(model, opts):
    from gru4rec_amd import evaluation
    which = ('recall', 'mrr').index(opts.primary_metric.lower())
    for fname in opts.test:
        print('Loading test data...')
        events = read_events(fname, opts, type(model))
        print('Starting evaluation (cut-off={}, using {} mode for tiebreaking)'.format(opts.measure, opts.eval_type))
        started = time.time()
        scores = evaluation.evaluate_gpu(model, events, batch_size=512, cut_off=opts.measure, mode=opts.eval_type,
                                         item_key=opts.item_key, session_key=opts.session_key, time_key=opts.time_key)
        print('Evaluation took {:.2f}s'.format(time.time() - started))
        for pos, cut in enumerate(opts.measure):
            print('Recall@{}: {:.6f} MRR@{}: {:.6f}'.format(cut, scores[0][pos], cut, scores[1][pos]))
        if opts.loglik:
            lm = evaluation.loglik_metrics(evaluation.loglik_gpu(model, events, temperature=opts.loglik_temperature, item_key=opts.item_key,
                                                                 session_key=opts.session_key, time_key=opts.time_key))
            print('NLL: {:.6f} Perplexity: {:.6f} Events: {} Ineligible: {}'.format(lm['nll'], lm['perplexity'], lm['n'], lm['n_ineligible']))
        if opts.log_primary_metric:
            print('PRIMARY METRIC: {}'.format(scores[which][0]))
        if opts.save_recs:
            import numpy as np
            recs = evaluation.recommend_gpu(model, events, k=opts.recs_k, batch_size=512, mode=opts.eval_type, item_key=opts.item_key,
                                            session_key=opts.session_key, time_key=opts.time_key)
            root, ext = os.path.splitext(opts.save_recs)
            out = opts.save_recs if len(opts.test) == 1 else '{}.{}{}'.format(root, opts.test.index(fname), ext or '.npz')
            np.savez(out, **recs)
            print('Saved the recommendations of {} events to: {}'.format(len(recs['rank']), out))
        if opts.save_audience:
            save_audience(model, events, opts, fname)


def save_audience(model, events, opts, fname):
    """--save_audience: the test sessions' full sequences (events of items the model does not know are dropped, as in the evaluation) are
    the histories of GRU4Rec.audience_sessions; the indices it returns are written as the sessions' ids."""
    import numpy as np
    if not hasattr(model, 'audience_sessions'):
        print('ERROR. The model class {} does not support --save_audience'.format(type(model).__module__))
        sys.exit(1)
    if not opts.audience_items:
        print('ERROR. --save_audience needs --audience_items FILE (one item id per line)')
        sys.exit(1)
    ids = dict(zip(model.itemidmap.index.astype(str), model.itemidmap.index))      # (a pickled table may hold ids that are not strings)
    with open(opts.audience_items, 'rt') as fh:
        wanted = [line.strip() for line in fh if line.strip()]
    unknown = [w for w in wanted if w not in ids]
    if unknown or not wanted:
        print('ERROR. --audience_items: {}'.format('the file is empty' if not wanted else 'the model does not know item {}'.format(unknown[0])))
        sys.exit(1)
    table = events[[opts.session_key, opts.item_key, opts.time_key]].copy()
    table[opts.item_key] = table[opts.item_key].astype(str)
    table = table[table[opts.item_key].isin(ids)].sort_values([opts.session_key, opts.time_key], kind='stable')
    sess = table[opts.session_key].values
    cuts = np.flatnonzero(sess[1:] != sess[:-1]) + 1
    items = np.array([ids[i] for i in table[opts.item_key]])
    histories = np.split(items, cuts)
    session_ids = sess[np.concatenate([[0], cuts]).astype(np.int64)]
    started = time.time()
    idx, values, counts = model.audience_sessions(histories, [ids[w] for w in wanted], opts.audience_k, by=opts.audience_by)
    root, ext = os.path.splitext(opts.save_audience)
    out = opts.save_audience if len(opts.test) == 1 else '{}.{}{}'.format(root, opts.test.index(fname), ext or '.npz')
    np.savez(out, item_ids=np.array([ids[w] for w in wanted]), session_ids=np.where(idx >= 0, session_ids[np.maximum(idx, 0)], -1), values=values,
             counts=counts)
    print('Saved the audiences ({}, k = {}) of {} items among {} sessions to: {} ({:.2f}s)'.format(opts.audience_by, opts.audience_k, len(wanted),
                                                                                               len(histories), out, time.time() - started))


def save_neighbors(model, opts):
    import numpy as np
    if not hasattr(model, 'item_neighbors'):
        print('ERROR. The model class {} does not support --save_neighbors'.format(type(model).__module__))
        sys.exit(1)
    started = time.time()
    ids, scores = model.item_neighbors(k=opts.neighbors_k, metric=opts.neighbors_metric)
    np.savez(opts.save_neighbors, item_ids=model.itemidmap.index.values, neighbor_ids=ids, scores=scores)
    print('Saved the {} nearest neighbours ({}) of {} items to: {} ({:.2f}s)'.format(opts.neighbors_k, opts.neighbors_metric, len(ids),
                                                                                   opts.save_neighbors, time.time() - started))


def main(argv=None):
    opts = build_parser().parse_args(argv)
    sources = [opts.parameter_string is not None, opts.parameter_file is not None, bool(opts.load_model)]
    if sum(sources) != 1:
        print('ERROR. Exactly one of the following parameters must be provided: --parameter_string, --parameter_file, --load_model')
        sys.exit(1)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if opts.gpus > 1 and 'WORLD_SIZE' not in os.environ and not opts.load_model:
        # become the launcher: N ranks of this very command line (rank 0 keeps stdout, the others' progress lines go to stderr)
        from gru4rec_amd import launch
        sys.exit(launch.spawn(__file__, sys.argv[1:] if argv is None else list(argv), opts.gpus))
    model_cls = importlib.import_module(opts.gru4rec_model).GRU4Rec
    if opts.load_model:
        print('Loading trained model from file: {}'.format(opts.path))
        model = model_cls.loadmodel(opts.path)
        if opts.item_groups:      # a loaded model gets its groups, and -s writes it back with them
            set_item_groups(model, opts.item_groups)
            if opts.save_model is not None:
                print('Saving the model to: {}'.format(opts.save_model))
                model.savemodel(opts.save_model)
    else:
        model = train(model_cls, opts)
    if opts.save_neighbors:
        save_neighbors(model, opts)
    if opts.test is not None:
        evaluate(model, opts)


if __name__ == '__main__':
    main()
